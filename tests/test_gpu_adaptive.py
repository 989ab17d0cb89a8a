"""GPU tests of adaptive sampling (psdr_jit_amd/adaptive.py, csrc/hip/adaptive.hip).

  1  counts, offsets and the pixel list against the Python-integer restatement of the rule (tests/test_adaptive_cpu.py::allocate): bit-equal
  2  the fold against a float64 segment mean, its repeatability, its transpose, torch.autograd through plan.merge
  3  render_c_adaptive: a uniform plan is the per-pixel mean of a plain renderC over the same list; the sample count of a skewed plan; opts.spp; the empty plan
  4  the differentiable recipe: renderD over plan.pix with batch_edges, plan.merge, backward()

The scan of the allocation has two levels (adaptive.hip): a tile of 2048 pixels per workgroup, and the sums of up to 8192 tiles added by every workgroup, 256 threads
striding over them.  Sizes: 1, 63, 64, 65 (one wave and its edges), 1025 (several waves of one tile), 2049 (just past one tile: the second level has two entries),
2048 * 257 + 1 (more tiles than the second level's stride of 256).  2^24, the largest n, needs no third level.

Bounds.  U = 2^-24 is the unit roundoff of float32.  A float32 sum of c terms, in ANY order, differs from the exact sum by at most (c - 1) U sum |terms| to first
order (every term passes through at most c - 1 additions, each with relative error <= U).  The fold adds the rows of a pixel so, evaluates the rest of its formula
in double and rounds once to float32 (one more U |out| <= U sum |terms|); the sample counts rows_n and base_n are small integers, exact in float32.  With the
base as one more term that is at most (c_p + 1) U sum |terms|, inside the (c_p + 2) U sum |terms| each element is held to."""
import os

import numpy as np
import pytest

import scenes
import test_adaptive_cpu as rule

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
SIZES = [1, 63, 64, 65, 1025, 2049]
BIG = 2048 * 257 + 1


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists)")
    import __graft_entry__
    __graft_entry__.build()
    import psdr_jit_amd
    return torch, psdr_jit_amd


def _check_plan(env, w, budget, min_count, label):
    torch, psdr = env
    plan = psdr.PixelPlan.from_weights(torch.from_numpy(w), budget, min_count)
    counts, offsets, _, _ = rule.allocate(w, budget, min_count)
    got_c, got_o, got_p = plan.counts.cpu().numpy(), plan.offsets.cpu().numpy(), plan.pix.cpu().numpy()
    assert plan.n == len(w) and plan.total == budget and got_c.dtype == np.int32 and got_o.dtype == np.int32 and got_p.dtype == np.int32
    assert np.array_equal(got_c, counts), (label, np.nonzero(got_c != counts)[0][:8])
    assert np.array_equal(got_o, offsets), (label, np.nonzero(got_o != offsets)[0][:8])
    assert np.array_equal(got_p, np.repeat(np.arange(len(w)), counts)), label


@pytest.mark.parametrize("n", SIZES)
def test_counts_offsets_and_list_equal_the_restatement(env, n):
    rng = np.random.default_rng(1000 + n)
    cases = 0
    for name, w in rule.weight_maps(n, rng).items():
        for min_count in (0, 2):
            for budget in rule.budgets(n, min_count):
                _check_plan(env, w, budget, min_count, (name, n, budget, min_count))
                cases += 1
    assert cases == (25 if n > 2 else 20)          # (min_count = 2 leaves the budget 7 n + 3 only: the others are below n * min_count, refused - tested below)


def test_counts_past_the_second_levels_stride(env):
    rng = np.random.default_rng(77)
    maps = rule.weight_maps(BIG, rng)
    _check_plan(env, maps["random"], 7 * BIG + 3, 2, "random")
    _check_plan(env, maps["bad"], BIG - 1, 0, "bad")
    _check_plan(env, maps["hot"], 7 * BIG + 3, 0, "hot")


def test_from_weights_refuses_what_the_entry_point_refuses(env):
    torch, psdr = env
    with pytest.raises(RuntimeError, match="n \\* min_count"):
        psdr.PixelPlan.from_weights(torch.ones(16), 31, 2)
    with pytest.raises(RuntimeError, match="negative"):
        psdr.PixelPlan.from_weights(torch.ones(16), -1)
    with pytest.raises(RuntimeError, match="psdr_hip_adaptive_counts"):
        psdr.PixelPlan.from_weights(torch.ones(0), 4)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the fold
def _manual_plan(env, counts):
    torch, psdr = env
    counts = np.asarray(counts, dtype=np.int32)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    pix = np.repeat(np.arange(len(counts)), counts).astype(np.int32)
    dev = "cuda"
    return psdr.PixelPlan(torch.from_numpy(counts).to(dev), torch.from_numpy(offsets).to(dev), torch.from_numpy(pix).to(dev), len(counts), int(offsets[-1])), pix


def _segment_counts(which, rng):
    if which == "mixed":                         # pixels without entries, single entries, segments longer than a wave
        c = rng.integers(0, 10, 37)
        c[[0, 5, 36]] = 0
        c[7], c[20] = 1, 200
        return c
    if which == "one pixel holds the list":
        return np.array([0, 0, 5003, 0, 0])
    return rng.integers(0, 150, 300)


def _fold64(counts, pix, rows, rows_n, base, base_n, square):
    """(the fold in float64 from the float32 inputs, the sum of the absolute terms of every element)"""
    n, ch = len(counts), rows.shape[1]
    n_tot = base_n + rows_n * counts.astype(np.float64)[:, None]
    safe = np.where(n_tot > 0, n_tot, 1.0)
    wr, wb = rows_n / safe, base_n / safe
    if square:
        wr, wb = wr * wr, wb * wb
    s, a = np.zeros((n, ch)), np.zeros((n, ch))
    np.add.at(s, pix, rows.astype(np.float64))
    np.add.at(a, pix, np.abs(rows.astype(np.float64)))
    b = base.astype(np.float64) if base is not None else np.zeros((n, ch))
    live = n_tot > 0
    return np.where(live, wb * b + wr * s, 0.0), np.where(live, wb * np.abs(b) + wr * a, 0.0)


@pytest.mark.parametrize("which", ["mixed", "one pixel holds the list", "many"])
@pytest.mark.parametrize("channels", [1, 3])
def test_fold_against_float64(env, which, channels):
    torch, psdr = env
    rng = np.random.default_rng(len(which) * 10 + channels)
    counts = _segment_counts(which, rng)
    plan, pix = _manual_plan(env, counts)
    rows = (rng.standard_normal((plan.total, channels)) * 10.0 ** rng.uniform(-2, 2, (plan.total, 1))).astype(np.float32)
    base = rng.standard_normal((plan.n, channels)).astype(np.float32)
    rows_t, base_t = torch.from_numpy(rows).cuda(), torch.from_numpy(base).cuda()
    for rows_n, base_n, use_base in ((4.0, 0.0, False), (4.0, 8.0, True), (1.0, 3.0, True)):
        for square in (0, 1):
            r = np.abs(rows) if square else rows
            b = (np.abs(base) if square else base) if use_base else None
            r_t = rows_t.abs() if square else rows_t
            b_t = (base_t.abs() if square else base_t) if use_base else None
            fold = (lambda: plan.merge_sq(r_t, rows_n, b_t, base_n)) if square else (lambda: plan.merge(r_t, rows_n, b_t, base_n))
            got_t = fold()
            got = got_t.cpu().numpy()
            want, terms = _fold64(counts, pix, r, rows_n, b, base_n, square)
            bound = (counts[:, None] + 2) * U * terms
            err = np.abs(got.astype(np.float64) - want)
            print("%s, %d channel(s), rows_n %g base_n %g square %d: largest error / bound %.3g" % (which, channels, rows_n, base_n, square, (err / np.maximum(bound, 1e-300)).max()))
            assert got.shape == (plan.n, channels) and got.dtype == np.float32
            assert np.all(err <= bound), (which, channels, rows_n, base_n, square, np.argwhere(err > bound)[:5])
            if not use_base:
                assert np.all(got[counts == 0] == 0.0)           # no entries, no base: exactly 0
            assert torch.equal(got_t, fold())                    # the order of every sum is fixed


def test_fold_transpose_and_autograd(env):
    torch, psdr = env
    rng = np.random.default_rng(31)
    counts = _segment_counts("mixed", rng)
    plan, pix = _manual_plan(env, counts)
    ch, rows_n, base_n = 3, 4.0, 8.0
    x = rng.standard_normal((plan.total, ch)).astype(np.float32)
    b = rng.standard_normal((plan.n, ch)).astype(np.float32)
    y = rng.standard_normal((plan.n, ch)).astype(np.float32)
    for use_base in (True, False):
        bn = base_n if use_base else 0.0
        rows = torch.from_numpy(x).cuda().requires_grad_()
        base = torch.from_numpy(b).cuda().requires_grad_() if use_base else None
        out = plan.merge(rows, rows_n, base, bn)
        (out * torch.from_numpy(y).cuda()).sum().backward()
        d_rows = rows.grad.cpu().numpy().astype(np.float64)
        d_base = base.grad.cpu().numpy().astype(np.float64) if use_base else np.zeros((plan.n, ch))
        # <merge(x, b), y> == <x, d_rows> + <b, d_base>.  The left side carries the fold's error, (c_p + 2) U sum |terms| per element, times |y|; every element of the
        # transpose is one product evaluated in double and rounded once, U |y_p| (weight): together (c_p + 3) U |y_p| sum |terms_p|
        _, terms = _fold64(counts, pix, x, rows_n, b if use_base else None, bn, 0)
        lhs = float((out.detach().cpu().numpy().astype(np.float64) * y).sum())
        rhs = float((x.astype(np.float64) * d_rows).sum() + (b.astype(np.float64) * d_base).sum())
        bound = float(((counts[:, None] + 3) * U * np.abs(y) * terms).sum())
        print("transpose, base %s: %.9g against %.9g, difference %.3g, bound %.3g" % (use_base, lhs, rhs, abs(lhs - rhs), bound))
        assert abs(lhs - rhs) <= bound
        # autograd against an index_add_ restatement in float64: each gradient element is one rounding of its exact value (2 U: the restatement rounds as well)
        rows64 = torch.tensor(x, dtype=torch.float64, requires_grad=True)
        base64 = torch.tensor(b, dtype=torch.float64, requires_grad=True)
        n_tot = bn + rows_n * torch.tensor(counts, dtype=torch.float64)[:, None]
        s = torch.zeros((plan.n, ch), dtype=torch.float64).index_add_(0, torch.from_numpy(pix).long(), rows64)
        out64 = torch.where(n_tot > 0, (bn * base64 + rows_n * s) / n_tot.clamp_min(1.0), torch.zeros_like(s))
        (out64 * torch.tensor(y, dtype=torch.float64)).sum().backward()
        assert np.all(np.abs(d_rows - rows64.grad.numpy()) <= 2 * U * np.abs(rows64.grad.numpy()))
        if use_base:
            assert np.all(np.abs(d_base - base64.grad.numpy()) <= 2 * U * np.abs(base64.grad.numpy()))
            assert np.abs(d_base).max() > 0
        assert np.abs(d_rows).max() > 0 and rows.grad.shape == rows.shape


# ---------------------------------------------------------------------------------------------------------------------------
# 3. render_c_adaptive
W, H = 32, 24


@pytest.fixture(scope="module")
def box(env):
    import product
    return product.build_scene(scenes.cbox_scene(W, H, spp=1, param="light_x"))


def test_uniform_plan_is_the_mean_of_a_plain_render_over_the_list(env, box):
    torch, psdr = env
    sc, n, k = box, W * H, 3
    integ = psdr.PathTracer(2)
    sc.opts.spp = 1
    sc.configure(sc.__dict__.get("_psdr_active", []))
    # min_count = k with budget = k W H leaves nothing for the weights to place: the plan is uniform whatever the pilot saw (it runs at another spp: the option is switched and restored)
    img, sq, plan = psdr.render_c_adaptive(integ, sc, k * n, seed=5, pilot_spp=4, min_count=k, reuse_pilot=False)
    assert sc.opts.spp == 1 and plan.total == k * n and plan.seed == 5 + (1 << 24)
    counts = plan.counts.cpu().numpy()
    pix = plan.pix.cpu().numpy()
    assert np.array_equal(counts, np.full(n, k)) and np.array_equal(pix, np.repeat(np.arange(n), k))
    rows = integ.renderC(sc, 0, seed=plan.seed, batch_pix=plan.pix).cpu().numpy()
    _, rows_sq = psdr.render_c_sq(integ, sc, 0, seed=plan.seed, batch_pix=plan.pix)
    want, terms = _fold64(counts, pix, rows, 1.0, None, 0.0, 0)
    want_sq, terms_sq = _fold64(counts, pix, rows_sq.cpu().numpy(), 1.0, None, 0.0, 1)
    assert np.abs(want - rows.astype(np.float64).reshape(n, k, 3).mean(axis=1)).max() <= 1e-12           # (the reference IS the per-pixel mean)
    err, err_sq = np.abs(img.cpu().numpy() - want), np.abs(sq.cpu().numpy() - want_sq)
    print("uniform plan: image error / bound %.3g, squares %.3g; mean image %.4g" % ((err / np.maximum((k + 2) * U * terms, 1e-300)).max(),
                                                                                    (err_sq / np.maximum((k + 2) * U * terms_sq, 1e-300)).max(), want.mean()))
    assert want.max() > 0 and np.all(err <= (k + 2) * U * terms) and np.all(err_sq <= (k + 2) * U * terms_sq)
    assert plan.samples(1).cpu().numpy().tolist() == [float(k)] * n
    var = plan.variance(img, sq, 1).cpu().numpy()
    assert np.isfinite(var).all() and var.max() > 0


def test_skewed_plan_spends_the_budget_and_restores_spp(env, box):
    torch, psdr = env
    sc, n = box, W * H
    integ = psdr.PathTracer(2)
    sc.opts.spp = 2
    sc.configure(sc.__dict__.get("_psdr_active", []))
    try:
        budget = 2 * (4 * n + 7)
        img, sq, plan = psdr.render_c_adaptive(integ, sc, budget, seed=9)
        counts = plan.counts.cpu().numpy()
        assert sc.opts.spp == 2 and plan.total == budget // 2 and counts.sum() == plan.total and counts.max() > counts.min()
        assert float(plan.samples(2, 2).double().sum()) == n * 2 + budget                      # the pilot's samples plus the budget
        # the result is the fold of the two renders it made
        pilot, pilot_sq = psdr.render_c_sq(integ, sc, 0, seed=9)
        rows, rows_sq = psdr.render_c_sq(integ, sc, 0, seed=plan.seed, batch_pix=plan.pix)
        pix = plan.pix.cpu().numpy()
        want, terms = _fold64(counts, pix, rows.cpu().numpy(), 2.0, pilot.cpu().numpy(), 2.0, 0)
        want_sq, terms_sq = _fold64(counts, pix, rows_sq.cpu().numpy(), 2.0, pilot_sq.cpu().numpy(), 2.0, 1)
        # (render_c_sq adds the two samples of a row or pixel with float atomics: one more U per input, (c_p + 1) terms)
        slack = (2 * counts[:, None] + 3) * U
        assert np.all(np.abs(img.cpu().numpy() - want) <= slack * terms) and np.all(np.abs(sq.cpu().numpy() - want_sq) <= slack * terms_sq)
        with pytest.raises(ValueError, match="multiple"):
            psdr.render_c_adaptive(integ, sc, budget + 1, seed=9)
        with pytest.raises(ValueError, match="seed"):
            psdr.render_c_adaptive(integ, sc, budget)
        # a way out through an exception: the pilot's spp does not stay behind
        with pytest.raises(Exception):
            psdr.render_c_adaptive(integ, sc, budget, sensor_id=99, seed=9, pilot_spp=4)
        assert sc.opts.spp == 2
    finally:
        sc.opts.spp = 1
        sc.configure(sc.__dict__.get("_psdr_active", []))


def test_empty_plan_returns_the_pilot_and_renders_no_list(env, box, monkeypatch):
    torch, psdr = env
    sc = box
    integ = psdr.PathTracer(2)
    calls = []
    plain = psdr.render_c_sq

    def counted(*a, **kw):
        calls.append(kw.get("batch_pix", -1))
        return plain(*a, **kw)
    monkeypatch.setattr(psdr, "render_c_sq", counted)
    img, sq, plan = psdr.render_c_adaptive(integ, sc, 0, seed=5, pilot_spp=2)
    assert len(calls) == 1 and isinstance(calls[0], int) and calls[0] == -1
    assert plan.total == 0 and plan.pix.numel() == 0 and int(plan.counts.abs().max()) == 0 and sc.opts.spp == 1
    sc.opts.spp = 2
    sc.configure(sc.__dict__.get("_psdr_active", []))
    try:
        pilot, pilot_sq = plain(integ, sc, 0, seed=5)
    finally:
        sc.opts.spp = 1
        sc.configure(sc.__dict__.get("_psdr_active", []))
    # (image and squares are sums of float atomics, two samples per pixel: another run of the same pilot agrees to their order, one U per addition)
    assert float(img.max()) > 0 and float((img - pilot).abs().max()) <= 2 * U * float(pilot.abs().max())
    assert float((sq - pilot_sq).abs().max()) <= 2 * U * float(pilot_sq.abs().max())
    with pytest.raises(ValueError, match="no sample"):
        psdr.render_c_adaptive(integ, sc, 0, seed=5, pilot_spp=2, reuse_pilot=False)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the differentiable recipe
def _moving_box_scene(psdr, P, width=24, height=16, spp=2):
    """the README box with the translation P of the small box as a leaf"""
    from psdr_jit_amd import Matrix4fC, Matrix4fD
    D = scenes.DATA
    sc = psdr.Scene()
    sc.opts.spp = sc.opts.sppe = sc.opts.sppse = spp
    sc.opts.width, sc.opts.height = width, height
    sc.opts.log_level = 0
    cam = psdr.PerspectiveCamera(60, 0.000001, 10000000.)
    cam.to_world = Matrix4fD([[1., 0., 0., 208.], [0., 1., 0., 273.], [0., 0., 1., -800.], [0., 0., 0., 1.]])
    sc.add_Sensor(cam)
    sc.add_BSDF(psdr.DiffuseBSDF([0.0, 0.0, 0.0]), "light")
    sc.add_BSDF(psdr.DiffuseBSDF([0.5, 0.5, 0.5]), "grey")
    sc.add_BSDF(psdr.DiffuseBSDF([0.95, 0.95, 0.95]), "white")
    I = np.eye(4, dtype=np.float32).tolist()
    sc.add_Mesh(os.path.join(D, "cbox_luminaire.obj"), Matrix4fC([[1., 0., 0., 0.], [0., 1., 0., -0.5], [0., 0., 1., 0.], [0., 0., 0., 1.]]), "light", psdr.AreaLight([20.0, 20.0, 8.0]))
    for f, b in (("cbox_smallbox", "grey"), ("cbox_largebox", "grey"), ("cbox_floor", "white"), ("cbox_back", "white")):
        sc.add_Mesh(os.path.join(D, f + ".obj"), Matrix4fC(I), b, None)
    sc.param_map["Mesh[1]"].set_transform(Matrix4fD([[1., 0., 0., P * 100.], [0., 1., 0., 0.], [0., 0., 1., 0.], [0., 0., 0., 1.]]))
    sc.configure()
    sc.configure([0])
    return sc


def test_differentiable_recipe(env):
    """renderD over plan.pix with the edge terms, plan.merge, backward(): P.grad against the same render folded by an index_add_ mean.

    Both gradients are sum_k <d_rows[k], d rows[k] / dP> through the same reverse pass.  The adjoints d_rows of the two folds are each within 2 U of w[p] / counts[p]
    (one division, one rounding), and the reverse pass adds its N samples' shares with float atomics in an order of its own in every run: the order-free bound
    (N - 1) U sum |shares|.  With A = sum_k,c |d_rows[k, c] d rows[k, c] / dP|, the sum of the absolute per-row contributions (from forward_grad), standing for
    the sum of the absolute shares, each gradient is within (N + 1) U A of the exact one and the two within 2 (N + 1) U A of each other; N = total * spp
    interior samples + W H (sppe + sppse) edge samples."""
    torch, psdr = env
    width, height, spp = 24, 16, 2
    n = width * height
    P = psdr.FloatD(0.).requires_grad_()
    sc = _moving_box_scene(psdr, P, width, height, spp)
    integ = psdr.PathTracer(2)
    rng = np.random.default_rng(3)
    plan = psdr.PixelPlan.from_weights(torch.from_numpy(rng.random(n).astype(np.float32) ** 4), 3 * n, min_count=1)
    counts = plan.counts.cpu().numpy()
    assert counts.min() >= 1 and counts.max() > 4 and counts.sum() == 3 * n
    w = torch.linspace(0.5, 1.5, n * 3, device="cuda").reshape(n, 3)

    rows = integ.renderD(sc, 0, seed=7, batch_pix=plan.pix, batch_edges=True)
    assert tuple(rows.shape) == (plan.total, 3)
    img = plan.merge(rows, spp)
    per_row = psdr.forward_grad(rows, P).detach().double() * (w / plan.counts[:, None]).double()[plan.pix.long()]
    A = float(per_row.abs().sum())
    (img * w).sum().backward(retain_graph=True)          # (the graph from P to the mesh transform is shared with the second render below)
    got = float(P.grad)
    P.grad = None

    rows2 = integ.renderD(sc, 0, seed=7, batch_pix=plan.pix, batch_edges=True)
    img2 = torch.zeros((n, 3), device="cuda").index_add_(0, plan.pix.long(), rows2) / plan.counts[:, None]
    assert float((img2.detach() - img.detach()).abs().max()) <= 2 * (int(counts.max()) + 2) * U * float(rows2.abs().max())           # (each mean within (c + 2) U max |rows|)
    (img2 * w).sum().backward()
    want = float(P.grad)
    N = plan.total * spp + n * 2 * spp
    tol = 2 * (N + 1) * U * A
    print("recipe: dP %.7g (plan.merge) against %.7g (index_add_), difference %.3g, bound %.3g; sum of the absolute per-row contributions %.4g" % (got, want, abs(got - want), tol, A))
    assert A > 0 and want != 0.0 and abs(float(per_row.sum()) - want) < 1e-2 * A          # a gradient that is there, and the one forward mode sees
    assert abs(got - want) <= tol
