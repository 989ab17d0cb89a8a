"""Per-pixel sums of squared sample contributions (psdr.render_c_sq / render_d_fwd_sq, psdr_hip_render_c_sq / psdr_hip_render_d_fwd_sq; DESIGN.md "Sample squares").

    sq[p, c] = the sum, over the samples of the launched terms, of (what the sample adds to img[p, c])^2,        d_sq: the same for d_img.

  1, 2  full frames against the oracle's per-lane radiances, scene in LDS (lock-step kernels) and BVH scene (decoupled kernels)
  3     a pixel list, image and interior derivative, sample by sample: the oracle with spp = 1 and every pixel repeated spp times IS the GPU's sample list
  4     image, derivative and sampler streams are those of the plain calls
  5     the shards of a call add up to the call, all four buffers, both shard modes
  6     the edge terms (no per-sample output in the oracle): the variance the squares predict against the variance across seeds

Bounds.  SQ_TOL = 2e-3: the project's oracle tolerance TOL = 1e-3 (tests/test_gpu_parity.py) propagated through a square to first order.  Cases 4 and 5 use
the bounds the project uses for results that differ by the order of the float atomics (tests/test_gpu_lean_kernels.py, tests/test_gpu_parity.py:216)."""
import ctypes as C

import numpy as np
import pytest

import product
import scenes

pytestmark = pytest.mark.gpu
SQ_TOL = 2e-3
TOL_IMAGE, TOL_DERIVATIVE = 2e-6, 2e-5
SEED_STRIDE = 100003


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists)")
    import __graft_entry__
    __graft_entry__.build()
    import psdr_jit_amd
    from psdr_jit_amd import cabi
    return torch, psdr_jit_amd, cabi


def _np(*tensors):
    return [t.cpu().numpy() for t in tensors]


def _lane_squares(lanes, spp):
    """float64 sums of (x / spp)^2 over the spp lanes of every pixel, non-finite lanes taken as 0 (the scrub of renderC); and which pixels have only zero lanes"""
    x = np.where(np.isfinite(lanes), lanes, 0.0).astype(np.float64).reshape(-1, spp, 3)
    return ((x / spp) ** 2).sum(axis=1), (x == 0.0).all(axis=1)


def _full_frame_against_lanes(env, orc, spec, label, some_dark):
    _, psdr, _ = env
    spp, n = spec.spp, spec.width * spec.height
    sc = product.build_scene(spec)
    integ = psdr.PathTracer(3)
    img, sq = _np(*psdr.render_c_sq(integ, sc, 0, seed=11))
    ref = orc.OracleScene(spec, [0])
    want_sq, dark = _lane_squares(ref.li_lanes(0, n * spp, max_depth=3, seed=11), spp)
    e_sq, e_img = product.rel_l2(sq, want_sq), product.rel_l2(img, ref.render_c(max_depth=3, seed=11))
    e_plain = product.rel_l2(img, integ.renderC(sc, 0, seed=11).cpu().numpy())
    print("%s: sq %.3g, image against the oracle %.3g, against renderC %.3g (max sq %.3g, %d of %d entries dark)" % (label, e_sq, e_img, e_plain, sq.max(), dark.sum(), dark.size))
    assert sq.shape == (n, 3) and np.isfinite(sq).all() and sq.max() > 0 and sq.min() >= 0
    assert np.all(sq[dark] == 0.0) and (dark.sum() > 0 or not some_dark)
    assert e_sq < SQ_TOL and e_img < SQ_TOL and e_plain < SQ_TOL


def test_full_frame_scene_in_lds(env, orc):
    _full_frame_against_lanes(env, orc, scenes.cbox_scene(32, 32, spp=4), "cbox 32 x 32", True)           # (most of this frame is background)


def test_full_frame_bvh_scene(env, orc):
    spec = scenes.config5_scene(48, 48, 4, 0, 0, level=1, env_res=(64, 32))
    assert sum(len(m.faces) for m in spec.meshes) > 64          # kBruteForceMax (scene_dev.h): a BVH scene, the decoupled path kernels
    _full_frame_against_lanes(env, orc, spec, "config 5, level 1, 48 x 48", False)


PIX = np.array([5, 37, 100, 200, 37], dtype=np.int32)            # (pixel 37 twice on purpose)


def _pixel_list_case(env, orc, param, integ_of, oracle_setup, hide_emitters, with_derivative):
    torch, psdr, _ = env
    spp = 4
    sc = product.build_scene(scenes.cbox_scene(16, 16, spp=spp, param=param))
    integ = integ_of(psdr)
    integ.hide_emitters = hide_emitters
    img, d_img, sq, d_sq = _np(*psdr.render_d_fwd_sq(integ, sc, 0, seed=13, batch_pix=torch.from_numpy(PIX), terms=psdr.TERM_INTERIOR))
    # the oracle's rows ARE the samples: row 4k + i is sample i of row k (lane 4k + i, seeded with seed + pix_ids[k] in both)
    ref = orc.OracleScene(scenes.cbox_scene(16, 16, spp=1, param=param), [0])
    oracle_setup(ref)
    rows, d_rows = ref.render_d(max_depth=integ.max_depth, hide_emitters=hide_emitters, seeds=(13, 13, 13), pix_ids=np.repeat(PIX, spp), terms=orc.TERM_INTERIOR)
    rows, d_rows = rows.astype(np.float64).reshape(-1, spp, 3), d_rows.astype(np.float64).reshape(-1, spp, 3)
    assert np.array_equal(rows[1], rows[4]) and np.array_equal(d_rows[1], d_rows[4])
    e_img, e_sq = product.rel_l2(img, rows.mean(axis=1)), product.rel_l2(sq, ((rows / spp) ** 2).sum(axis=1))
    print("pixel list, %s: image %.3g sq %.3g" % (param, e_img, e_sq))
    assert sq.shape == (len(PIX), 3) and sq.max() > 0
    assert e_img < SQ_TOL and e_sq < SQ_TOL
    if with_derivative:
        want_dsq = ((d_rows / spp) ** 2).sum(axis=1)
        e_d, e_dsq = product.rel_l2(d_img, d_rows.mean(axis=1)), product.rel_l2(d_sq, want_dsq)
        print("pixel list, %s: derivative %.3g d_sq %.3g (max d_sq %.3g)" % (param, e_d, e_dsq, d_sq.max()))
        assert d_sq.max() > 0 and want_dsq.max() > 0
        assert np.all(d_sq[want_dsq == 0.0] == 0.0)
        assert e_d < SQ_TOL and e_dsq < SQ_TOL


@pytest.mark.parametrize("param", ["albedo", "light_x"])
def test_pixel_list_per_sample(env, orc, param):
    _pixel_list_case(env, orc, param, lambda psdr: psdr.PathTracer(3), lambda ref: None, False, True)


def test_pixel_list_direct_integrator(env, orc):
    _pixel_list_case(env, orc, "albedo", lambda psdr: psdr.Direct(2), lambda ref: ref.set_direct_mis(2), False, False)


def test_pixel_list_hide_emitters(env, orc):
    _pixel_list_case(env, orc, "albedo", lambda psdr: psdr.PathTracer(3), lambda ref: None, True, False)


@pytest.fixture(scope="module")
def cbox(env):
    return product.build_scene(scenes.cbox_scene(32, 32, 4, 4, 4, param="light_x"))


@pytest.fixture(scope="module")
def blob(env):
    return product.build_scene(scenes.config5_scene(48, 48, 4, 4, 4, level=1, env_res=(64, 32), param="blob_x"))


@pytest.mark.parametrize("terms", [7, 1, 2, 4])
@pytest.mark.parametrize("which", ["cbox", "blob"])
def test_nothing_else_moved(env, request, which, terms):
    """image and derivative of the _sq call against the plain call (other kernels - general instead of lean, the secondary-edge kernel with the squares -, same samples),
    and the sampler streams after it: exactly the plain call's, so a following seed=-1 renderC gives the same image"""
    _, psdr, _ = env
    sc = request.getfixturevalue(which)
    integ = psdr.PathTracer(3)
    img, d_img = _np(*psdr.render_d_fwd(integ, sc, 0, seed=31, terms=terms))
    state = [sc._sampler_state(k) for k in range(3)]
    after = integ.renderC(sc, 0).cpu().numpy()
    img_s, d_img_s, sq, d_sq = _np(*psdr.render_d_fwd_sq(integ, sc, 0, seed=31, terms=terms))
    assert [sc._sampler_state(k) for k in range(3)] == state
    after_s = integ.renderC(sc, 0).cpu().numpy()
    e_d, e_after = product.rel_l2(d_img_s, d_img), product.rel_l2(after_s, after)
    print("%s terms %d: derivative %.3g, the next renderC %.3g (max |d| %.3g, max d_sq %.3g)" % (which, terms, e_d, e_after, np.abs(d_img).max(), d_sq.max()))
    assert np.abs(d_img).max() > 0 and d_sq.max() > 0 and d_sq.min() >= 0
    assert e_d < TOL_DERIVATIVE and e_after < TOL_IMAGE
    if terms & 1:
        e_img = product.rel_l2(img_s, img)
        print("%s terms %d: image %.3g" % (which, terms, e_img))
        assert e_img < TOL_IMAGE and sq.max() > 0
    else:
        assert np.abs(img).max() == 0.0 and np.abs(img_s).max() == 0.0 and sq.max() == 0.0          # the edge terms have no primal


@pytest.mark.parametrize("which", ["cbox", "blob"])
def test_render_c_sq_leaves_render_c_alone(env, request, which):
    _, psdr, _ = env
    sc = request.getfixturevalue(which)
    integ = psdr.PathTracer(3)
    img = integ.renderC(sc, 0, seed=33).cpu().numpy()
    state = [sc._sampler_state(k) for k in range(3)]
    after = integ.renderC(sc, 0).cpu().numpy()
    img_s, sq = _np(*psdr.render_c_sq(integ, sc, 0, seed=33))
    assert [sc._sampler_state(k) for k in range(3)] == state
    after_s = integ.renderC(sc, 0).cpu().numpy()
    e_img, e_after = product.rel_l2(img_s, img), product.rel_l2(after_s, after)
    print("%s: image %.3g, the next renderC %.3g" % (which, e_img, e_after))
    assert sq.max() > 0 and e_img < TOL_IMAGE and e_after < TOL_IMAGE


@pytest.mark.parametrize("shard_mode", [0, 1])
def test_shards_add_up(env, cbox, shard_mode):
    torch, _, cabi = env
    n = 32 * 32

    def run(rank, count):
        buf = torch.empty((4, n, 3), dtype=torch.float32, device="cuda")
        a = cabi.make_args(max_depth=2, seeds=(4, 4, 4), shard_rank=rank, shard_count=count, shard_mode=shard_mode)
        cabi.check(cabi.lib().psdr_hip_render_d_fwd_sq(cbox._hip_handle(), C.byref(a), buf[0].data_ptr(), buf[1].data_ptr(), buf[2].data_ptr(), buf[3].data_ptr(), None))
        torch.cuda.synchronize()
        return buf.cpu().numpy().astype(np.float64)
    full = run(0, 1)
    halves = [run(0, 2), run(1, 2)]
    parts = halves[0] + halves[1]
    errs = [product.rel_l2(parts[k], full[k]) for k in range(4)]
    print("shard mode %d: image %.3g derivative %.3g sq %.3g d_sq %.3g" % (shard_mode, errs[0], errs[1], errs[2], errs[3]))
    assert all(np.abs(h[k]).max() > 0 for h in halves for k in range(4))
    assert errs[0] < 1e-6 and errs[2] < 1e-6 and errs[1] < 1e-5 and errs[3] < 1e-5


EDGE_K = {"primary": 128, "secondary": 32}
# the oracle alone, seeds 0, 100003, 2 x 100003, ...: V_emp of four disjoint sets of K seeds
#   secondary, K = 32 (128 renders)   0.05890 0.05546 0.05131 0.05386   mean 0.05488, sample standard deviation / mean = 0.0579
#   primary,   K = 32 (128 renders)   0.04902 0.05249 0.06450 0.04491   mean 0.05273, s = 0.1600: 3 s = 0.48, next to the limit of 0.5 -> K raised
#   primary,   K = 128 (512 renders)  0.05256 0.06044 0.06005 0.05609   mean 0.05729, s = 0.0648
S_PRIMARY, S_SECONDARY = 0.0648, 0.0579


@pytest.mark.parametrize("term", ["primary", "secondary"])
def test_edge_terms_against_the_variance_across_seeds(env, orc, term):
    """V_pred = mean over seeds of sum_{p,c} variance_from_sq(d_img, d_sq, W H sppe), one GPU render per seed, against V_emp = sum_{p,c} of the variance of the
    oracle's d_img across the same K = EDGE_K[term] seeds.  The band: |V_pred / V_emp - 1| < 3 s with s = the relative spread (sample standard deviation / mean) of V_emp over
    four disjoint sets of K seeds, from oracle renders made for this purpose (table above): s = 0.0648 (primary, K = 128: at K = 32 the band would be 0.48, so K was
    raised, not the band) and 0.0579 (secondary, K = 32); the bands are 0.194 and 0.174, inside the factor of 1.5 the check must keep.  (A wrong normalisation is off by
    sppe, sppe^2 or 2.)  The seeds are k x 100003, k = 0..K-1.  An edge sample's distribution is heavy-tailed: among 128 seeds counted from 1 instead of 0, one
    secondary-edge frame holds a single sample of 5.8e3 against a V_emp of 0.055, and s of such a set says nothing - s is a property of the seeds used here."""
    _, psdr, _ = env
    s_rel = {"primary": S_PRIMARY, "secondary": S_SECONDARY}[term]
    assert 3 * s_rel < 0.5                                       # the band stays inside a factor of 1.5
    spec = scenes.cbox_scene(32, 32, spp=1, sppe=16, param="box_x") if term == "primary" else scenes.cbox_scene(32, 32, spp=1, sppse=16, param="box_x")
    t = psdr.TERM_PRIMARY if term == "primary" else psdr.TERM_SECONDARY
    sc = product.build_scene(spec)
    ref = orc.OracleScene(spec, [0])
    integ = psdr.PathTracer(1)
    n = psdr.samples_behind(sc, t)
    assert n == 32 * 32 * 16
    seeds = [k * SEED_STRIDE for k in range(EDGE_K[term])]
    pred, frames = [], []
    for seed in seeds:
        img, d_img, sq, d_sq = psdr.render_d_fwd_sq(integ, sc, 0, seed=seed, terms=t)
        pred.append(float(psdr.variance_from_sq(d_img.double(), d_sq.double(), n).sum()))
        frames.append(ref.render_d(max_depth=1, seeds=(seed, seed, seed), terms=t)[1].astype(np.float64))
    v_pred, v_emp = float(np.mean(pred)), float(np.var(np.stack(frames), axis=0, ddof=1).sum())
    print("%s edges: V_pred %.4g V_emp %.4g ratio %.4f, band 3 s = %.3f" % (term, v_pred, v_emp, v_pred / v_emp, 3 * s_rel))
    assert v_emp > 0 and abs(v_pred / v_emp - 1.0) < 3 * s_rel
