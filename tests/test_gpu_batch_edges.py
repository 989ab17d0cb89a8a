"""Edge terms of batch-pixel renderD (renderD(..., batch_pix=pix, batch_edges=True); psdr_hip_render_d_fwd_batch / _bwd_batch) on the GPU.

The contract: row k of the derivative = the interior derivative of row k as a pixel list has always had it + the FULL-FRAME primary- and
secondary-edge derivative of pixel pix[k] (same seeds, lane counts, scaling, guiding, sharding as the full-frame call).  That gives the
feature an exact checker: the oracle's full-frame edge terms, gathered at pix.

Tolerances are the project's own, none of them taken from what this code gives:
   TOL = 1e-3 rel-L2 against the oracle (test_gpu_parity.py, BASELINE north_star);
   1e-5 rel-L2 where the same samples are summed in another order (test_gpu_parity.py::test_shards_sum_to_full_frame);
   2e-3 * max(1, |want|) for reverse mode against forward mode / against the full-frame reverse mode (test_gpu_api.py::test_batch_render_reverse_mode).
A list only tests something where the reference is non-zero on it: every (scene, term, list) asserts at least MIN_NONZERO pixels of the
list on which the oracle's term is non-zero (counted on the CPU oracle when the lists were chosen; the assertion fails, it does not skip)."""
import ctypes as C
import os

import numpy as np
import pytest

import adjoint_buffers
import product
import scenes

pytestmark = pytest.mark.gpu
TOL = 1e-3
ORDER_TOL = 1e-5
MIN_NONZERO = 16
PRIMARY, SECONDARY, INTERIOR, ALL = 2, 4, 1, 7


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists)")
    return torch


@pytest.fixture(scope="module")
def psdr():
    import __graft_entry__
    __graft_entry__.build()
    import psdr_jit_amd
    return psdr_jit_amd


def _crop(w=64, h=64):
    """rows h/4 .. 3h/4, columns w/8 .. 5w/8 (64 x 64: rows 16-47 x columns 8-39), row-major"""
    return np.arange(w * h).reshape(h, w)[h // 4:3 * h // 4, w // 8:5 * w // 8].reshape(-1).astype(np.int32)


def _rand(w=64, h=64):
    """an eighth of the frame (64 x 64: 512 pixels) drawn without replacement"""
    return np.random.default_rng(5).choice(w * h, (w * h) // 8, replace=False).astype(np.int32)


def _lower_half(w=64, h=64):
    return np.arange(w * h).reshape(h, w)[h // 2:].reshape(-1).astype(np.int32)


LISTS = {"crop": _crop, "rand": _rand, "lower": _lower_half}


def _nonzero_rows(a):
    return int((np.abs(np.asarray(a)).max(axis=1) > 0).sum())


def _check_rows(got, want, what):
    """`want` = the oracle's full-frame term gathered at the list: enough of it is non-zero, and the batch rows match it"""
    nz = _nonzero_rows(want)
    err = product.rel_l2(got, want)
    print("%s: %d non-zero reference pixels of %d, rel-L2 %.3g" % (what, nz, len(want), err))
    assert nz >= MIN_NONZERO, "%s: only %d pixels of the list carry a non-zero reference" % (what, nz)
    assert err < TOL, (what, err)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. against the oracle, per term (brute-force box, PathTracer(2))
ORACLE_CASES = [("camera_x", PRIMARY, "crop"), ("camera_x", PRIMARY, "rand"), ("camera_x", SECONDARY, "crop"), ("camera_x", SECONDARY, "rand"),
                ("light_x", SECONDARY, "crop"), ("light_x", SECONDARY, "rand"), ("box_x", PRIMARY, "crop")]


@pytest.mark.parametrize("param,term,which", ORACLE_CASES)
def test_edge_term_of_a_pixel_list_matches_oracle(torch_cuda, psdr, orc, param, term, which):
    spec = scenes.cbox_scene(64, 64, 8, 8, 8, param=param)
    sc = product.build_scene(spec)
    ref = orc.OracleScene(spec, [0])
    pix = LISTS[which]()
    _, want_full = ref.render_d(max_depth=2, seeds=(21, 21, 21), terms=term)
    img, dimg = psdr.render_d_fwd(psdr.PathTracer(2), sc, 0, seed=21, batch_pix=torch_cuda.from_numpy(pix), batch_edges=True, terms=term)
    assert tuple(dimg.shape) == (len(pix), 3) and float(img.abs().max()) == 0.0          # edge terms have zero primal
    _check_rows(dimg.cpu().numpy(), want_full[pix], "%s term %d %s" % (param, term, which))


@pytest.mark.parametrize("which", ["crop", "rand"])
def test_all_terms_of_a_pixel_list_match_oracle(torch_cuda, psdr, orc, which):
    """terms = ALL: today's interior rows of the list (the oracle's batch mode) plus the two gathered full-frame edge terms"""
    spec = scenes.cbox_scene(64, 64, 8, 8, 8, param="camera_x")
    sc = product.build_scene(spec)
    ref = orc.OracleScene(spec, [0])
    pix = LISTS[which]()
    want_img, want_int = ref.render_d(max_depth=2, seeds=(21, 21, 21), pix_ids=pix)          # (a pixel list in the oracle: interior only)
    _, want_p = ref.render_d(max_depth=2, seeds=(21, 21, 21), terms=PRIMARY)
    _, want_s = ref.render_d(max_depth=2, seeds=(21, 21, 21), terms=SECONDARY)
    assert _nonzero_rows(want_p[pix]) >= MIN_NONZERO and _nonzero_rows(want_s[pix]) >= MIN_NONZERO
    img, dimg = psdr.render_d_fwd(psdr.PathTracer(2), sc, 0, seed=21, batch_pix=torch_cuda.from_numpy(pix), batch_edges=True)
    assert product.rel_l2(img.cpu().numpy(), want_img) < TOL
    _check_rows(dimg.cpu().numpy(), want_int + want_p[pix] + want_s[pix], "camera_x all terms " + which)
    # ... and the edge share is not a rounding matter: without it the rows are far from the reference
    _, d_int = psdr.render_d_fwd(psdr.PathTracer(2), sc, 0, seed=21, batch_pix=torch_cuda.from_numpy(pix))
    assert product.rel_l2(d_int.cpu().numpy(), want_int) < TOL
    assert product.rel_l2(d_int.cpu().numpy(), want_int + want_p[pix] + want_s[pix]) > 10 * TOL


# ---------------------------------------------------------------------------------------------------------------------------
# 2. exact relations, no oracle
def test_exact_relations_with_the_full_frame(torch_cuda, psdr, orc):
    torch = torch_cuda
    W = H = 64
    n = W * H
    spec = scenes.cbox_scene(W, H, 8, 8, 8, param="camera_x")
    sc = product.build_scene(spec)
    integ = psdr.PathTracer(2)
    _, full_e = psdr.render_d_fwd(integ, sc, 0, seed=21, terms=PRIMARY | SECONDARY)
    full_e = full_e.cpu().numpy()
    assert _nonzero_rows(full_e) >= 10 * MIN_NONZERO
    # the identity list: image and derivative are the full-frame call's.  The interior lanes coincide at spp = 1 - a lane of a pixel list is seeded with
    # seed + pixel, a full-frame lane with seed + lane (integrator.cpp:24-28), and lane == pixel only then; with more samples per pixel the interior
    # term of the identity list is another estimate of the same image, as it has always been - so this relation runs on the 1 / 8 / 8 box
    ident = torch.arange(n, dtype=torch.int32)
    sc1 = product.build_scene(scenes.cbox_scene(W, H, 1, 8, 8, param="camera_x"))
    full1_img, full1_d = (t.cpu().numpy() for t in psdr.render_d_fwd(integ, sc1, 0, seed=21))
    img, d = psdr.render_d_fwd(integ, sc1, 0, seed=21, batch_pix=ident, batch_edges=True)
    assert product.rel_l2(img.cpu().numpy(), full1_img) < ORDER_TOL and product.rel_l2(d.cpu().numpy(), full1_d) < ORDER_TOL
    _, d1_int = psdr.render_d_fwd(integ, sc1, 0, seed=21, batch_pix=ident)
    assert product.rel_l2(d1_int.cpu().numpy(), full1_d) > 10 * TOL                       # (the edge share is what made them equal)
    # ... at 8 / 8 / 8 the edge share of the identity list is the full frame's
    _, d = psdr.render_d_fwd(integ, sc, 0, seed=21, batch_pix=ident, batch_edges=True, terms=PRIMARY | SECONDARY)
    assert product.rel_l2(d.cpu().numpy(), full_e) < ORDER_TOL
    # a random permutation, edge terms only: row k is full-frame row pix[k]
    perm = np.random.default_rng(11).permutation(n).astype(np.int32)
    _, d = psdr.render_d_fwd(integ, sc, 0, seed=21, batch_pix=torch.from_numpy(perm), batch_edges=True, terms=PRIMARY | SECONDARY)
    assert product.rel_l2(d.cpu().numpy(), full_e[perm]) < ORDER_TOL
    # duplicates: every copy of a pixel carries the same edge share (the copies are interleaved with the first occurrences)
    crop = _crop(W, H)
    dup = np.concatenate([crop[::3], crop, crop[::5][::-1]]).astype(np.int32)
    _, d = psdr.render_d_fwd(integ, sc, 0, seed=21, batch_pix=torch.from_numpy(dup), batch_edges=True, terms=PRIMARY | SECONDARY)
    d = d.cpu().numpy()
    assert _nonzero_rows(full_e[dup]) >= MIN_NONZERO and product.rel_l2(d, full_e[dup]) < ORDER_TOL
    first = {}
    for k, p in enumerate(dup):
        first.setdefault(int(p), k)
    rep = np.array([first[int(p)] for p in dup])
    assert (rep != np.arange(len(dup))).sum() > 100 and np.array_equal(d, d[rep])
    # a list that misses every edge pixel: the pixels on which the full-frame edge terms are exactly zero receive exactly zero
    miss = np.nonzero(np.abs(full_e).max(axis=1) == 0)[0].astype(np.int32)
    assert len(miss) >= 256
    img, d = psdr.render_d_fwd(integ, sc, 0, seed=21, batch_pix=torch.from_numpy(miss), batch_edges=True, terms=PRIMARY | SECONDARY)
    assert float(d.abs().max()) == 0.0 and float(img.abs().max()) == 0.0


def test_switch_off_is_todays_behaviour_and_sampler_streams(torch_cuda, psdr, orc):
    torch = torch_cuda
    spec = scenes.cbox_scene(64, 64, 8, 8, 8, param="camera_x")
    sc = product.build_scene(spec)
    integ = psdr.PathTracer(2)
    pix = torch.from_numpy(_crop())
    a_img, a_d = psdr.render_d_fwd(integ, sc, 0, seed=21, batch_pix=pix)                         # the call as it has always been written
    a_state = [sc._sampler_state(k) for k in range(3)]
    b_img, b_d = psdr.render_d_fwd(integ, sc, 0, seed=21, batch_pix=pix, batch_edges=False)
    b_state = [sc._sampler_state(k) for k in range(3)]
    assert torch.equal(a_img, b_img) and torch.equal(a_d, b_d) and a_state == b_state
    # switch off: the edge samplers are seeded with the full-frame counts and do not advance (today's values)
    n_full = 64 * 64
    assert [tuple(s) for s in a_state[1:]] == [(True, n_full * 8, 21, 0), (True, n_full * 8, 21, 0)]
    # switch on: they advance as in the full-frame call
    psdr.render_d_fwd(integ, sc, 0, seed=21)
    full_state = [sc._sampler_state(k) for k in range(3)]
    c_img, _ = psdr.render_d_fwd(integ, sc, 0, seed=21, batch_pix=pix, batch_edges=True)
    c_state = [sc._sampler_state(k) for k in range(3)]
    assert c_state[1] == full_state[1] and c_state[2] == full_state[2] and full_state[1][3] > 0 and full_state[2][3] == 3
    assert c_state[0][3] == full_state[0][3] and c_state[0][1] == len(pix) * 8               # interior: the list's lanes, the same draws per lane
    assert product.rel_l2(c_img.cpu().numpy(), a_img.cpu().numpy()) < 1e-6                      # the primal image does not see the edge terms
    # "advance only" bits (terms >> 4): nothing launched for the edge terms, their samplers move all the same
    pix_dev, scratch = pix.cuda(), torch.zeros((2, len(pix), 3), dtype=torch.float32, device="cuda")
    integ._renderD(sc, 0, 21, pix_dev.data_ptr(), len(pix), scratch[0].data_ptr(), scratch[1].data_ptr(), 0, 0, 1, INTERIOR | (ALL << 4), True)
    torch.cuda.synchronize()
    assert [sc._sampler_state(k) for k in range(3)] == c_state and float(scratch[1].abs().max()) > 0
    integ._renderD(sc, 0, 21, pix_dev.data_ptr(), len(pix), scratch[0].data_ptr(), scratch[1].data_ptr(), 0, 0, 1, INTERIOR | (ALL << 4), False)
    torch.cuda.synchronize()
    assert [sc._sampler_state(k) for k in range(3)] == a_state
    # the switch without a list
    with pytest.raises(ValueError, match="batch_pix"):
        psdr.render_d_fwd(integ, sc, 0, seed=21, batch_edges=True)
    with pytest.raises(ValueError, match="batch_pix"):
        integ.renderD(sc, 0, seed=21, batch_edges=True)
    from psdr_jit_amd import cabi
    buf = torch.zeros((2, n_full, 3), dtype=torch.float32, device="cuda")
    a = cabi.make_args(max_depth=2, seeds=(21, 21, 21))
    assert cabi.lib().psdr_hip_render_d_fwd_batch(sc._hip_handle(), C.byref(a), buf[0].data_ptr(), buf[1].data_ptr(), None) != 0
    assert b"pix_ids" in cabi.lib().psdr_hip_last_error()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. reverse mode
def _pose_scene(psdr, tx, P, refl, res=40, spp=8):
    """the README box with a camera translation tx, a translation P of the small box and the colour refl of the boxes as leaves"""
    from psdr_jit_amd import Matrix4fC, Matrix4fD
    D = scenes.DATA
    sc = psdr.Scene()
    sc.opts.spp = sc.opts.sppe = sc.opts.sppse = spp
    sc.opts.width = sc.opts.height = res
    sc.opts.log_level = 0
    cam = psdr.PerspectiveCamera(60, 0.000001, 10000000.)
    cam.to_world = Matrix4fD([[1., 0., 0., 208. + tx * 50.], [0., 1., 0., 273.], [0., 0., 1., -800.], [0., 0., 0., 1.]])
    sc.add_Sensor(cam)
    sc.add_BSDF(psdr.DiffuseBSDF([0.0, 0.0, 0.0]), "light")
    sc.add_BSDF(psdr.DiffuseBSDF(), "cat")
    sc.add_BSDF(psdr.DiffuseBSDF([0.95, 0.95, 0.95]), "white")
    I = np.eye(4, dtype=np.float32).tolist()
    sc.add_Mesh(os.path.join(D, "cbox_luminaire.obj"), Matrix4fC([[1., 0., 0., 0.], [0., 1., 0., -0.5], [0., 0., 1., 0.], [0., 0., 0., 1.]]), "light", psdr.AreaLight([20.0, 20.0, 8.0]))
    for f, b in (("cbox_smallbox", "cat"), ("cbox_largebox", "cat"), ("cbox_floor", "white"), ("cbox_back", "white")):
        sc.add_Mesh(os.path.join(D, f + ".obj"), Matrix4fC(I), b, None)
    sc.param_map["Mesh[1]"].set_transform(Matrix4fD([[1., 0., 0., P * 100.], [0., 1., 0., 0.], [0., 0., 1., 0.], [0., 0., 0., 1.]]))
    sc.param_map["BSDF[id=cat]"].reflectance = refl
    sc.configure()
    sc.configure([0])
    return sc


@pytest.mark.parametrize("which", ["crop", "duplicates"])
def test_backward_equals_forward_grad_with_edge_terms(torch_cuda, psdr, orc, which):
    """loss.backward() on a batch image with the edge terms on == <w, forward_grad> for a mesh translation, the camera pose and a colour"""
    torch = torch_cuda
    tx = psdr.FloatD(0.).requires_grad_()
    P = psdr.FloatD(0.).requires_grad_()
    refl = torch.tensor([0.5, 0.5, 0.5], requires_grad=True)
    sc = _pose_scene(psdr, tx, P, refl)
    pix = _crop(40, 40)
    if which == "duplicates":
        pix = np.concatenate([pix[::2], pix, pix[::7]]).astype(np.int32)
    integ = psdr.PathTracer(2)
    # the interior-only image of the same list, for the size of the edge share
    img0 = integ.renderD(sc, 0, seed=7, batch_pix=pix)
    w = torch.linspace(0.5, 1.5, img0.numel(), device=img0.device).reshape(img0.shape)
    int_P, int_t = float((psdr.forward_grad(img0, P) * w).sum()), float((psdr.forward_grad(img0, tx) * w).sum())
    img = integ.renderD(sc, 0, seed=7, batch_pix=pix, batch_edges=True)
    assert tuple(img.shape) == (len(pix), 3) and product.rel_l2(img.detach().cpu().numpy(), img0.detach().cpu().numpy()) < 1e-6
    dirc = torch.tensor([1.0, -0.5, 0.25])
    want_P = float((psdr.forward_grad(img, P) * w).sum())
    want_t = float((psdr.forward_grad(img, tx) * w).sum())
    want_r = float((psdr.forward_grad(img, refl, direction=dirc) * w).sum())
    (img * w).sum().backward()
    got_P, got_t, got_r = float(P.grad), float(tx.grad), float((refl.grad * dirc).sum())
    print("%s: box %.6g / %.6g (interior only %.6g), camera %.6g / %.6g (interior only %.6g), colour %.6g / %.6g" % (which, got_P, want_P, int_P, got_t, want_t, int_t, got_r, want_r))
    assert abs(want_P - int_P) > 1e-2 and abs(want_t - int_t) > 1e-2             # the edge terms are in the derivative
    assert abs(got_P - want_P) < 2e-3 * max(1.0, abs(want_P)), (got_P, want_P)
    assert abs(got_t - want_t) < 2e-3 * max(1.0, abs(want_t)), (got_t, want_t)
    assert abs(want_r) > 1e-3 and abs(got_r - want_r) < 2e-3 * max(1.0, abs(want_r)), (got_r, want_r)


def _bwd_buffers(torch, cabi, sc, spec, fn, args, w):
    g, bufs, _ = adjoint_buffers.allocate(sc, spec, ("g_camera",))
    cabi.check(fn(sc._hip_handle(), C.byref(args), w.data_ptr(), C.byref(g), None))
    torch.cuda.synchronize()
    return adjoint_buffers.to_f64(bufs)


@pytest.mark.parametrize("scene", ["cbox", "sphere"])
def test_batch_backward_equals_full_frame_backward_with_scattered_weights(torch_cuda, psdr, orc, scene):
    """Independent of the new forward path: with terms = PRIMARY | SECONDARY the adjoints from weights w[k] on the list equal those of the
    FULL-FRAME reverse pass with Wp = sum_k w[k] [pix[k] == p] - the same samples, only the order of the sums differs.
    (brute-force box: record-free closed form in LDS tables; sphere box: the two-stage BVH pipeline)"""
    torch = torch_cuda
    from psdr_jit_amd import cabi
    res = 48
    spec = scenes.cbox_scene(res, res, 8, 8, 8, param="box_x") if scene == "cbox" else scenes.sphere_scene(res, res, 8, 8, 8)
    sc = product.build_scene(spec)
    crop = _crop(res, res)
    pix = np.concatenate([crop, crop[::4], _rand(res, res)]).astype(np.int32)               # duplicates inside and across the parts
    pix_t = torch.from_numpy(pix).cuda()
    gen = torch.Generator(device="cpu").manual_seed(3)
    w = (torch.rand((len(pix), 3), generator=gen) + 0.5).cuda()
    Wp = torch.zeros((res * res, 3), dtype=torch.float32, device="cuda").index_add_(0, pix_t.long(), w)
    L = cabi.lib()
    a_full = cabi.make_args(max_depth=2, seeds=(7, 8, 9), terms=PRIMARY | SECONDARY)
    a_list = cabi.make_args(max_depth=2, seeds=(7, 8, 9), terms=PRIMARY | SECONDARY, pix_ids_ptr=pix_t.data_ptr(), n_pix=len(pix))
    want = _bwd_buffers(torch, cabi, sc, spec, L.psdr_hip_render_d_bwd, a_full, Wp)
    got = _bwd_buffers(torch, cabi, sc, spec, L.psdr_hip_render_d_bwd_batch, a_list, w)
    old = _bwd_buffers(torch, cabi, sc, spec, L.psdr_hip_render_d_bwd, a_list, w)            # the old entry point keeps its interior-only batch behaviour
    for name in ("g_triangles", "g_sec_edges", "g_prim_edges", "g_camera"):
        diff, scale = np.abs(got[name] - want[name]).max(), np.abs(want[name]).max()
        print("%s %s: max |batch - full| = %.3g at max |full| = %.3g" % (scene, name, diff, scale))
        assert diff < 2e-3 * max(1.0, scale), (name, diff, scale)
        assert np.abs(old[name]).max() == 0.0
    assert np.abs(want["g_prim_edges"]).max() > 0 and np.abs(want["g_sec_edges"]).max() > 0 and np.abs(want["g_triangles"]).max() > 0


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the other forms of the kernels
@pytest.mark.parametrize("term", [PRIMARY, SECONDARY])
def test_bvh_scene_matches_oracle(torch_cuda, psdr, orc, term):
    """the sphere box: BVH traversal, the decoupled path kernel and the two-stage secondary-edge pipeline"""
    spec = scenes.sphere_scene(64, 64, 8, 8, 8)
    sc = product.build_scene(spec)
    ref = orc.OracleScene(spec, [0])
    pix = _lower_half()
    _, want_full = ref.render_d(max_depth=2, seeds=(21, 21, 21), terms=term)
    _, dimg = psdr.render_d_fwd(psdr.PathTracer(2), sc, 0, seed=21, batch_pix=torch_cuda.from_numpy(pix), batch_edges=True, terms=term)
    _check_rows(dimg.cpu().numpy(), want_full[pix], "sphere box term %d lower half" % term)


def test_direct_integrator_primary_edges_match_oracle(torch_cuda, psdr, orc):
    spec = scenes.cbox_scene(64, 64, 8, 8, 8, param="camera_x")
    sc = product.build_scene(spec)
    ref = orc.OracleScene(spec, [0])
    ref.set_direct_mis(2)
    pix = _crop()
    _, want_full = ref.render_d(max_depth=1, seeds=(21, 21, 21), terms=PRIMARY)
    _, dimg = psdr.render_d_fwd(psdr.Direct(2), sc, 0, seed=21, batch_pix=torch_cuda.from_numpy(pix), batch_edges=True, terms=PRIMARY)
    _check_rows(dimg.cpu().numpy(), want_full[pix], "Direct(2) primary crop")


def test_orthographic_camera_primary_edges_match_oracle(torch_cuda, psdr, orc):
    spec = scenes.ortho_cbox_scene(64, 64, 8, 8, 8, param="camera_x")
    sc = product.build_scene(spec)
    ref = orc.OracleScene(spec, [0])
    pix = _crop()
    _, want_full = ref.render_d(max_depth=2, seeds=(21, 21, 21), terms=PRIMARY)
    _, dimg = psdr.render_d_fwd(psdr.PathTracer(2), sc, 0, seed=21, batch_pix=torch_cuda.from_numpy(pix), batch_edges=True, terms=PRIMARY)
    _check_rows(dimg.cpu().numpy(), want_full[pix], "orthographic box primary crop")


def test_guided_secondary_edges_match_oracle(torch_cuda, psdr, orc):
    """guiding on (the set-up of test_gpu_parity.py::test_guiding_matches_oracle, at 64 x 64 with the camera as the parameter)"""
    spec = scenes.cbox_scene(64, 64, 8, 0, 8, param="camera_x")
    sc = product.build_scene(spec)
    ref = orc.OracleScene(spec, [0])
    integ = psdr.PathTracer(1)
    reso = [40, 4, 4, 16]
    integ.preprocess_secondary_edges(sc, 0, reso, 2, 5)
    g = ref.guiding_build(0, reso, nrounds=2, seed=5)
    pix = _crop()
    _, want_full = ref.render_d(max_depth=1, seeds=(6, 6, 6), terms=SECONDARY, guiding=g)
    _, dimg = psdr.render_d_fwd(integ, sc, 0, seed=6, batch_pix=torch_cuda.from_numpy(pix), batch_edges=True, terms=SECONDARY)
    _check_rows(dimg.cpu().numpy(), want_full[pix], "guided secondary crop")


# ---------------------------------------------------------------------------------------------------------------------------
# 5. sharding at the C ABI
@pytest.mark.parametrize("shard_mode", [0, 1])
def test_shards_of_a_batch_call_sum_to_the_unsharded_call(torch_cuda, psdr, orc, shard_mode):
    torch = torch_cuda
    from psdr_jit_amd import cabi
    spec = scenes.cbox_scene(48, 48, 8, 8, 8, param="camera_x")
    sc = product.build_scene(spec)
    crop = _crop(48, 48)
    pix = np.concatenate([crop, crop[::4]]).astype(np.int32)
    pix_t = torch.from_numpy(pix).cuda()

    def run(rank, count, terms=ALL):
        buf = torch.empty((2, len(pix), 3), dtype=torch.float32, device="cuda")
        a = cabi.make_args(max_depth=2, seeds=(4, 4, 4), shard_rank=rank, shard_count=count, shard_mode=shard_mode, pix_ids_ptr=pix_t.data_ptr(), n_pix=len(pix), terms=terms)
        cabi.check(cabi.lib().psdr_hip_render_d_fwd_batch(sc._hip_handle(), C.byref(a), buf[0].data_ptr(), buf[1].data_ptr(), None))
        return buf.cpu().numpy()
    full = run(0, 1)
    parts = sum(run(r, 3) for r in range(3))
    assert product.rel_l2(parts[0], full[0]) < 1e-6 and product.rel_l2(parts[1], full[1]) < ORDER_TOL
    edge = run(0, 1, PRIMARY | SECONDARY)[1]
    edge_parts = [run(r, 3, PRIMARY | SECONDARY)[1] for r in range(3)]
    assert _nonzero_rows(edge) >= MIN_NONZERO and product.rel_l2(sum(edge_parts), edge) < ORDER_TOL
    assert all(_nonzero_rows(e) > 0 for e in edge_parts)                 # every rank carries a share of the edge samples
