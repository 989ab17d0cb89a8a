"""The early side switch of the primary-edge term (paths.h THE EARLY SIDE SWITCH, csrc/hip/edge_switch.h): a lane whose first path is known to have ended before the
vertex of the hit in hand is built switches to the sample's second path ahead of the loop's one make_its; the lanes that still read that vertex (a last hit on an
emitter, every camera hit at max_depth 0) switch one iteration later.  Rays, sampler draws and per-sample arithmetic are those of the late switch, which the counted
kernels keep - so every frame below is rendered twice in this process with the same seeds,

  through psdr_hip_render_d_fwd (the early switch; psdr_hip_render_d_fwd_batch for the pixel list) and through psdr_hip_render_d_fwd_counted (the late switch),

and the two derivative images agree to 1e-6 relative L2 (the same samples; only the order of the float atomics differs - tests/test_gpu_group_start.py measured 6.4e-8
for that kind of difference), and the early one equals the oracle's at 1e-3, the bound of the other parity files.  Every derivative compared is non-zero on the oracle.

The frames: the README box at 16 x 16 with 1 and 5 edge samples per pixel (one fetch batch, five) and at 24 x 16 with 3 (a partial last batch); max_depth 0, 1, 3, 6;
hide_emitters; a camera at z = -2600 (silhouettes against the void: camera rays miss); a camera under the luminaire looking up (camera hits and last hits on the
emitter: the detour); an orthographic sensor (the general kernel, the second path's origin from the cold rows); two
shards; a continuing sampler; skip_static_edges; a pixel list; and the three terms together once.  Reverse mode: psdr_hip_render_d_bwd with the primary-edge term
alone, <w, J v> with J v from the oracle against <J^T w, v>, as tests/test_gpu_adjoint.py checks its rows.

The early switch is compiled into the class-1 kernels only (the scene in LDS, Diffuse BSDFs).  The Microfacet box is class 3, which keeps the late switch in every
kernel (LABNOTES: with the early switch two RoughDielectric frames of the randomised parity run left the oracle's bound): its frame compares the late switch with itself
and exercises none of the new code - it stays as a check that class 3 still renders what the oracle does.
"""
import ctypes as C

import numpy as np
import pytest

import adjoint_buffers
import product
import scenes

pytestmark = pytest.mark.gpu
TOL_ORACLE = 1e-3
TOL_SAME_SAMPLES = 1e-6
SEEDS = (41, 42, 43)
PRIMARY = 2
FAR_Z = -2600.0                     # the README camera stands at z = -800


def _box(w, h, sppe, param="box_x", spp=0, sppse=0):
    return scenes.cbox_scene(w, h, spp, sppe, sppse, param=param)


def _far():
    spec = _box(32, 32, 4)
    spec.cameras[0].to_world_raw = np.asarray(scenes.translate(208.0, 273.0, FAR_Z), np.float32)
    return spec


def _look_up():
    """from under the luminaire, along +y: its four edges lie against the ceiling in the middle of the frame"""
    spec = _box(24, 24, 4, param="light_x")
    spec.cameras[0].to_world_raw = (scenes.translate(278.0, 150.0, 279.5) @ scenes._rot_x(-0.5 * np.pi)).astype(np.float32)
    return spec


# case -> (scene, max_depth, further psdr_render_args fields, terms)
CASES = {
    "16x16x1": (lambda: _box(16, 16, 1), 3, {}, PRIMARY),
    "16x16x5": (lambda: _box(16, 16, 5), 3, {}, PRIMARY),
    "24x16x3": (lambda: _box(24, 16, 3), 3, {}, PRIMARY),
    "depth0": (lambda: _box(24, 16, 3, param="light_x"), 0, {}, PRIMARY),          # (the first hit's Le is the whole path: only the luminaire's edges count)
    "depth1": (lambda: _box(24, 16, 3), 1, {}, PRIMARY),
    "depth6": (lambda: _box(24, 16, 3), 6, {}, PRIMARY),
    "hide": (lambda: _box(16, 16, 5, param="light_x"), 3, {"hide_emitters": True}, PRIMARY),
    "light_x": (lambda: _box(16, 16, 5, param="light_x"), 3, {}, PRIMARY),
    "far": (_far, 3, {}, PRIMARY),
    "look_up": (_look_up, 3, {}, PRIMARY),
    "look_up_depth0": (_look_up, 0, {}, PRIMARY),
    "look_up_depth1": (_look_up, 1, {}, PRIMARY),
    "microfacet": (lambda: scenes.microfacet_cbox_scene(16, 16, 0, 5, 0, param="box_x"), 3, {}, PRIMARY),          # (class 3: the late switch on both sides, see above)
    "ortho": (lambda: scenes.ortho_cbox_scene(16, 16, 0, 5, 0, param="box_x"), 3, {}, PRIMARY),
    "shard0": (lambda: _box(16, 16, 5), 3, {"shard_rank": 0, "shard_count": 2}, PRIMARY),
    "shard1": (lambda: _box(16, 16, 5), 3, {"shard_rank": 1, "shard_count": 2}, PRIMARY),
    "skip": (lambda: _box(16, 16, 5), 3, {"skips": (1000, 500, 250)}, PRIMARY),
    "static": (lambda: _box(16, 16, 5), 3, {"skip_static_edges": True}, PRIMARY),
    "all_terms": (lambda: _box(16, 16, 5, spp=5, sppse=5), 3, {}, 7),
}


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


def _render(env, sc, n_rows, depth, terms, counted=False, pix=None, **kw):
    """-> [2, n_rows, 3] (image, derivative); counted: the late switch"""
    torch, _, cabi = env
    buf = torch.zeros((2, n_rows, 3), dtype=torch.float32, device="cuda")
    if pix is not None:
        kw = dict(kw, pix_ids_ptr=pix.data_ptr(), n_pix=int(pix.numel()))
    a = cabi.make_args(max_depth=depth, seeds=SEEDS, terms=terms, **kw)
    h = C.c_void_p(sc._hip_handle())
    if counted:
        c = cabi.Counters()
        cabi.check(cabi.lib().psdr_hip_render_d_fwd_counted(h, C.byref(a), buf[0].data_ptr(), buf[1].data_ptr(), C.byref(c), None))
    elif pix is not None:
        cabi.check(cabi.lib().psdr_hip_render_d_fwd_batch(h, C.byref(a), buf[0].data_ptr(), buf[1].data_ptr(), None))
    else:
        cabi.check(cabi.lib().psdr_hip_render_d_fwd(h, C.byref(a), buf[0].data_ptr(), buf[1].data_ptr(), None))
    torch.cuda.synchronize()
    return buf.cpu().numpy()


def _oracle_d(orc, spec, depth, kw, terms):
    ref = orc.OracleScene(spec, [0])
    return ref.render_d(max_depth=depth, hide_emitters=bool(kw.get("hide_emitters", False)), seeds=SEEDS, skips=kw.get("skips", (0, 0, 0)), terms=terms,
                        shard_rank=kw.get("shard_rank", 0), shard_count=kw.get("shard_count", 1))


@pytest.mark.parametrize("name", list(CASES))
def test_early_switch_equals_the_late_switch_and_the_oracle(env, orc, name):
    make, depth, kw, terms = CASES[name]
    spec = make()
    sc = product.build_scene(spec)
    n = spec.width * spec.height
    early = _render(env, sc, n, depth, terms, **kw)
    late = _render(env, sc, n, depth, terms, counted=True, **kw)
    # (skip_static_edges leaves out samples whose contribution is zero; the oracle traces them all and gets the same frame)
    want_img, want_d = _oracle_d(orc, spec, depth, kw, terms)
    e_same, e_orc = product.rel_l2(early[1], late[1]), product.rel_l2(early[1], want_d)
    print("%s: early against late %.3g, against the oracle %.3g (max |d| %.3g)" % (name, e_same, e_orc, np.abs(want_d).max()))
    assert np.abs(want_d).max() > 0 and np.abs(late[1]).max() > 0, name
    if terms & 1:
        e_img = (product.rel_l2(early[0], late[0]), product.rel_l2(early[0], want_img))
        print("%s: image, early against late %.3g, against the oracle %.3g" % (name, *e_img))
        assert e_img[0] <= TOL_SAME_SAMPLES and e_img[1] < TOL_ORACLE, (name, e_img)
    else:
        assert np.abs(early[0]).max() == 0.0           # the edge terms have no primal
    assert e_same <= TOL_SAME_SAMPLES, (name, e_same)
    assert e_orc < TOL_ORACLE, (name, e_orc)


def test_pixel_list(env, orc):
    """the edge terms of a pixel list are the full frame's, gathered: against the counted full-frame launch and the oracle's full frame at the listed pixels"""
    torch = env[0]
    spec = _box(24, 16, 3)
    sc = product.build_scene(spec)
    n = spec.width * spec.height
    rng = np.random.default_rng(5)
    ids = np.concatenate([rng.integers(0, n, 150), np.arange(n // 2, n // 2 + 40)]).astype(np.int32)
    rng.shuffle(ids)
    pix = torch.from_numpy(ids).cuda()
    early = _render(env, sc, int(ids.size), 3, PRIMARY, pix=pix)
    late = _render(env, sc, n, 3, PRIMARY, counted=True)
    _, want_d = _oracle_d(orc, spec, 3, {}, PRIMARY)
    e_same, e_orc = product.rel_l2(early[1], late[1][ids]), product.rel_l2(early[1], want_d[ids])
    print("pixel list: early against late %.3g, against the oracle %.3g (max |d| %.3g)" % (e_same, e_orc, np.abs(want_d[ids]).max()))
    assert np.abs(want_d[ids]).max() > 0
    assert e_same <= TOL_SAME_SAMPLES and e_orc < TOL_ORACLE


@pytest.mark.parametrize("param", ["box_x", "light_x"])
def test_reverse_mode_primary_edges_against_the_oracle(env, orc, param):
    """<w, d_img> with d_img from the ORACLE's forward mode of the primary-edge term against <J^T w, v> from psdr_hip_render_d_bwd (the general kernel, early switch)"""
    torch, _, cabi = env
    spec = _box(16, 16, 5, param=param)
    sc = product.build_scene(spec)
    snap = sc._snapshot()
    d_tri = np.asarray(snap["d_triangles"], np.float64)
    d_sec = np.asarray(snap["d_sec_edges"], np.float64)[:, :6]
    d_prim = np.asarray(sc.param_map["Sensor[0]"]._primary_edges(True), np.float64)[:, :4]
    _, d_img = _oracle_d(orc, spec, 3, {}, PRIMARY)
    gen = torch.Generator(device="cpu").manual_seed(3)
    w = (torch.rand((spec.width * spec.height, 3), generator=gen) + 0.5).to("cuda")
    lhs = float((d_img.astype(np.float64) * w.cpu().numpy().astype(np.float64)).sum())
    scale = float((np.abs(d_img).astype(np.float64) * w.cpu().numpy().astype(np.float64)).sum()) + 1e-12
    g, bufs, _ = adjoint_buffers.allocate(sc, spec)
    a = cabi.make_args(max_depth=3, seeds=SEEDS, terms=PRIMARY)
    cabi.check(cabi.lib().psdr_hip_render_d_bwd(sc._hip_handle(), C.byref(a), w.data_ptr(), C.byref(g), None))
    torch.cuda.synchronize()
    g_tri, g_bsdf, g_em, g_sec, g_prim = [bufs[f].cpu().numpy().astype(np.float64) for f in adjoint_buffers.ROWS]
    rhs = (g_prim[:d_prim.shape[0]] * d_prim).sum()
    others = (g_tri * d_tri).sum() + (g_sec[:d_sec.shape[0]] * d_sec).sum() + np.abs(g_bsdf).sum() + np.abs(g_em).sum()
    print("reverse mode, %s: <w, J v> %.9g, <J^T w, v> %.9g, scale %.3g" % (param, lhs, rhs, scale))
    assert others == 0.0                                 # the primary-edge term moves the edge table only
    assert abs(lhs) > 1e-6 and abs(lhs - rhs) <= 1e-3 * scale, (param, lhs, rhs, scale)
