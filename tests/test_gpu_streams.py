"""Every GPU entry point on a side stream behind a delay (tests/stream_cases.py has the technique: a delayed producer, with decoys).

All other GPU tests run on the default stream, where a launch, clear or copy that goes to the wrong stream is ordered anyway.  Here every case runs under
`with torch.cuda.stream(S):` in two forms - the delay on S (catches work of the call that left S and runs too early) and the delay on the default stream (catches
work of the call that went to the null stream and lands too late) - and is held against the reference and the bound its entry point's own test uses, evaluated on
the TRUE inputs; the buffers hold valid decoys until the producer, queued behind the delay, overwrites them.

  1  forward renders: renderC, renderD (terms 7), render_c_sq, the batch-pixel form with edge terms; LDS, LDS with materials, BVH (the only class whose renderD forks)
  2  reverse mode: the image's adjoint produced behind the delay; box, BVH scene, and deep paths whose records are allocated inside the first backward
  3  guiding_build        4  ray batches: intersect, intersectAD forward and adjoint, trace / trace_pairs, env_sample / env_pdf
  5  two streams, one scene (ScratchGuard)        6  configure() between streams
  7  handles made under one stream and applied under another: Denoiser, VarianceDenoiser, Subdivision, LaplacianPreconditioner
  8  adaptive sampling: counts, expand, merge, merge_adj

Bounds are the existing ones: TOL = 1e-3 against the oracle (test_gpu_parity.py, test_gpu_batch_edges.py), SQ_TOL = 2e-3 (test_gpu_sample_squares.py), 2e-6 / 2e-5 between
two runs of the same samples whose float atomics add in another order (test_gpu_configs.py, test_gpu_lean_kernels.py), 2e-3 max(1, |want|) for reverse against forward
mode (test_gpu_api.py), 1e-6 against a freshly built scene (test_gpu_configure.py), and the derived bounds of test_gpu_denoise.py, test_gpu_vdenoise.py,
test_gpu_subdiv.py, test_gpu_precond.py and test_gpu_adaptive.py.  Where those tests assert bit equality between two runs, the run on S must give the bits of the same
call on the default stream.

The self-check (`not event.query()` when the call returns: the delay was still running) holds for every entry that returns without synchronising.  It is skipped, and said
so at the call, for those that synchronise inside: guiding_build, the create calls, the preconditioner's solve, a backward() through the Python layer (it reads the
adjoint buffers back), configure() - and for every case that goes through torch's backward(): the engine hands the node to its device thread and waits for it on the
host, and how long that takes is not this library's (8.5 ms once, in the middle of the whole suite).

Measured on an MI355X (tests/stream_cases.py): the slowest covered case is issued in ENQUEUE_MS = 0.4 ms, the delay is 4 ms; the 36 cases take 5 s together."""
import ctypes as C

import numpy as np
import pytest

import denoise_ref
import product
import scenes
import stream_cases as sc_
import subdiv_ref
import vdenoise_ref
from stream_cases import Slot, run_on_stream, run_plain

pytestmark = pytest.mark.gpu
TOL = 1e-3
SQ_TOL = 2e-3
TOL_IMAGE, TOL_DERIVATIVE = 2e-6, 2e-5
MIN_NONZERO = 16
U = 2.0 ** -24
FORMS = sc_.FORMS


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


@pytest.fixture(scope="module")
def streams(env):
    torch = env[0]
    return torch.cuda.Stream(), torch.cuda.Stream()


def _cpu(*tensors):
    return [t.detach().cpu().numpy() for t in tensors]


def _ptr(torch):
    return int(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. forward renders
DEPTH = 2
SCENES = {
    "lds": lambda: scenes.cbox_scene(32, 32, 2, 2, 2, param="camera_x"),
    "lds_materials": lambda: scenes.microfacet_cbox_scene(32, 32, 2, 2, 2, param="box_x"),
    "bvh": lambda: scenes.config5_scene(32, 32, 2, 2, 2, level=1, env_res=(64, 32), param="blob_x"),
}
_BUILT = {}


def _scene(env, orc, name):
    """(spec, product scene, oracle scene, oracle results) per scene class, built and rendered by the oracle once"""
    if name not in _BUILT:
        spec = SCENES[name]()
        ref = orc.OracleScene(spec, [0])
        n = spec.width * spec.height
        pix = np.random.default_rng(5).permutation(n).astype(np.int32)          # every pixel once, in random order (at 2 / 2 / 2 samples a shorter list meets too few edge samples)
        want = {"c": ref.render_c(max_depth=DEPTH, seed=7), "d": ref.render_d(max_depth=DEPTH, seeds=(9, 9, 9)), "pix": pix,
                "lanes": ref.li_lanes(0, n * spec.spp, max_depth=DEPTH, seed=7)}
        b_img, b_int = ref.render_d(max_depth=DEPTH, seeds=(21, 21, 21), pix_ids=pix)          # (a pixel list in the oracle: interior only)
        edges = ref.render_d(max_depth=DEPTH, seeds=(21, 21, 21), terms=orc.TERM_PRIMARY)[1] + ref.render_d(max_depth=DEPTH, seeds=(21, 21, 21), terms=orc.TERM_SECONDARY)[1]
        want["batch"] = (b_img, b_int + edges[pix], int((np.abs(edges[pix]).max(axis=1) > 0).sum()))
        _BUILT[name] = (spec, product.build_scene(spec), ref, want)
    return _BUILT[name]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", list(SCENES))
def test_forward_renders(env, orc, streams, name, form, monkeypatch):
    torch, psdr, cabi = env
    S = streams[0]
    spec, sc, ref, want = _scene(env, orc, name)
    integ = psdr.PathTracer(DEPTH)
    spp = spec.spp
    assert (sum(len(m.faces) for m in spec.meshes) > 64) == (name == "bvh")          # kBruteForceMax (scene_dev.h): the BVH path, whose renderD forks its edge terms
    pix = Slot(torch, want["pix"])
    # every entry once on the default stream: the first call of a kind loads its kernels and grows the scene's scratch, for which it may wait for its stream
    # (include/psdr_hip.h) - the self-check below is about the calls that follow; and it is what the runs on S are compared with
    plain_c = run_plain(torch, [], lambda: integ.renderC(sc, 0, seed=7), lambda t: t.cpu().numpy())
    plain_d = run_plain(torch, [], lambda: psdr.render_d_fwd(integ, sc, 0, seed=9), lambda o: _cpu(*o))
    plain_sq = run_plain(torch, [], lambda: psdr.render_c_sq(integ, sc, 0, seed=7), lambda o: _cpu(*o))
    plain_b = run_plain(torch, [pix], lambda: psdr.render_d_fwd(integ, sc, 0, seed=21, batch_pix=pix.buf, batch_edges=True), lambda o: _cpu(*o))
    # renderC
    got = run_on_stream(torch, S, form, [], lambda: integ.renderC(sc, 0, seed=7), lambda t: t.cpu().numpy())
    assert np.isfinite(got).all() and product.rel_l2(got, want["c"]) < TOL, (name, "renderC")
    assert product.rel_l2(got, plain_c) < TOL_IMAGE
    # renderD, forward mode, terms 7
    img, dimg = run_on_stream(torch, S, form, [], lambda: psdr.render_d_fwd(integ, sc, 0, seed=9), lambda o: _cpu(*o))
    assert product.rel_l2(img, plain_d[0]) < TOL_IMAGE and product.rel_l2(dimg, plain_d[1]) < TOL_DERIVATIVE
    assert np.abs(want["d"][1]).max() > 0
    assert product.rel_l2(img, want["d"][0]) < TOL and product.rel_l2(dimg, want["d"][1]) < TOL, (name, "renderD")
    if name == "bvh":
        # the forked call (edge terms on the scene's side streams, joined into S) against the three terms one after the other on the default stream
        with sc_.env_var(monkeypatch, "PSDR_NO_FORK", "1"):
            s_img, s_dimg = run_plain(torch, [], lambda: psdr.render_d_fwd(integ, sc, 0, seed=9), lambda o: _cpu(*o))
        assert product.rel_l2(img, s_img) < TOL_IMAGE and product.rel_l2(dimg, s_dimg) < TOL_DERIVATIVE
    # render_c_sq
    img, sq = run_on_stream(torch, S, form, [], lambda: psdr.render_c_sq(integ, sc, 0, seed=7), lambda o: _cpu(*o))
    x = np.where(np.isfinite(want["lanes"]), want["lanes"], 0.0).astype(np.float64).reshape(-1, spp, 3)
    assert product.rel_l2(img, want["c"]) < SQ_TOL and product.rel_l2(sq, ((x / spp) ** 2).sum(axis=1)) < SQ_TOL, (name, "render_c_sq")
    assert product.rel_l2(img, plain_sq[0]) < TOL_IMAGE
    # the batch-pixel form with edge terms: the pixel list is produced behind the delay, over the same ids in another order
    b_img, b_d, nonzero = want["batch"]
    assert nonzero >= MIN_NONZERO, "%s: only %d pixels of the list carry a non-zero edge reference" % (name, nonzero)
    img, dimg = run_on_stream(torch, S, form, [pix], lambda: psdr.render_d_fwd(integ, sc, 0, seed=21, batch_pix=pix.buf, batch_edges=True), lambda o: _cpu(*o))
    assert product.rel_l2(img, b_img) < TOL and product.rel_l2(dimg, b_d) < TOL, (name, "batch")
    assert product.rel_l2(img, plain_b[0]) < TOL_IMAGE and product.rel_l2(dimg, plain_b[1]) < TOL_DERIVATIVE
    stale = run_plain(torch, [], lambda: psdr.render_d_fwd(integ, sc, 0, seed=21, batch_pix=pix._decoy, batch_edges=True), lambda o: _cpu(*o))
    assert product.rel_l2(stale[1], b_d) > 10 * TOL          # (a call that read the decoy list is far from the reference: the case can fail)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. reverse mode
def _leaf_scene(env, name):
    """the scene of `name` with the translation of Mesh[0] (box: the luminaire, README.md:87-90; BVH: the blob) as a torch leaf P; d/dP is the spec's tangent"""
    torch, psdr, _ = env
    spec = scenes.cbox_scene(32, 32, 2, 2, 2, param="light_x") if name == "lds" else SCENES[name]()
    sc = product.build_scene(spec)
    P = psdr.FloatD(0.).requires_grad_()
    sc.param_map["Mesh[0]"].set_transform(psdr.Matrix4fD([[1., 0., 0., P * 100.], [0., 1., 0., 0.], [0., 0., 1., 0.], [0., 0., 0., 1.]]))
    sc.configure([0])
    return spec, sc, P


def _weights(n, seed=3):
    return (np.random.default_rng(seed).random((n, 3)) + 0.5).astype(np.float32)


def _backward(psdr, integ, sc, P, w_buf, seed):
    P.grad = None
    img = integ.renderD(sc, 0, seed=seed)
    img.backward(w_buf, retain_graph=True)          # loss = <w, img>; (the graph from P to the mesh transform is shared by the calls of a test)
    return P.grad.detach().clone()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["lds", "bvh"])
def test_reverse_mode(env, orc, streams, name, form):
    """loss.backward() under S, loss = <w, img> with w produced behind the delay: dP against <w, d img / dP> of the oracle's forward mode.  (backward() reads the adjoint
    buffers back to the host: it synchronises inside, no self-check.)

    Not bit for bit against the default stream: the reverse pass adds its samples' shares with float atomics in an order of its own in every launch, so two runs on the
    DEFAULT stream already differ (measured on an MI355X, box scene: -70.4197388, -70.4197235, -70.4197311 in three runs; tests/test_gpu_denoise.py states the same of
    its render).  No test of the suite asserts run-to-run bit equality of a render's adjoint, and none is asserted here: the run on S is held to the oracle and to the
    default stream's run at the bound of reverse against forward mode."""
    torch, psdr, _ = env
    spec, sc, P = _leaf_scene(env, name)
    integ = psdr.PathTracer(DEPTH)
    w = Slot(torch, _weights(spec.width * spec.height))
    _, wd = orc.OracleScene(spec, [0]).render_d(max_depth=DEPTH, seeds=(5, 5, 5))
    want = float((wd.astype(np.float64) * w.true_np).sum())
    stale = float((wd.astype(np.float64) * sc_.decoy_of(w.true_np)).sum())
    got = float(run_on_stream(torch, streams[0], form, [w], lambda: _backward(psdr, integ, sc, P, w.buf, 5), lambda g: g.cpu(), returns_early=False))
    base = float(run_plain(torch, [w], lambda: _backward(psdr, integ, sc, P, w.buf, 5), lambda g: g.cpu()))
    print("%s, delay on %s: dP %.9g, default stream %.9g, oracle %.9g (with the decoy weights %.9g)" % (name, form, got, base, want, stale))
    assert abs(want) > 1e-3 and abs(stale - want) > 2 * 2e-3 * max(1.0, abs(want))          # (the decoy is told apart at the bound)
    assert abs(got - want) < 2e-3 * max(1.0, abs(want))
    assert abs(base - want) < 2e-3 * max(1.0, abs(want)) and abs(got - base) < 2e-3 * max(1.0, abs(base))


@pytest.mark.parametrize("form", FORMS)
def test_reverse_mode_deep_paths_allocate_their_records_under_the_stream(env, orc, streams, form):
    """max_depth 6 under an environment map with a textured floor (the scene of test_gpu_api.py::test_reverse_mode_deep_paths_and_many_lookups): the per-lane records do
    not fit LDS, so the FIRST backward of a fresh scene allocates and clears `adj_rec` inside the call - under S.  Texel and radiance gradients against forward mode
    (which makes no such allocation), at that test's bound."""
    import os
    torch, psdr, _ = env
    rng = np.random.default_rng(23)
    spec = scenes.textured_scene(32, 32, 8, 0, 0, texture=scenes.checker_texture(8, 8), env=True)
    env0 = scenes.synthetic_envmap(32, 16)
    rad = torch.tensor(env0, requires_grad=True)
    tex = torch.tensor(spec.bsdfs[0].texture, requires_grad=True)
    sc = psdr.Scene()
    sc.opts.spp, sc.opts.sppe, sc.opts.sppse = 8, 0, 0
    sc.opts.width = sc.opts.height = 32
    sc.opts.log_level = 0
    cam = psdr.PerspectiveCamera(60, 0.000001, 10000000.)
    cam.to_world = psdr.Matrix4fD(np.asarray(spec.cameras[0].to_world_raw).tolist())
    sc.add_Sensor(cam)
    sc.add_BSDF(psdr.DiffuseBSDF(tex), "tex")
    sc.add_BSDF(psdr.DiffuseBSDF([0.8, 0.7, 0.6]), "cat")
    floor = psdr.Mesh()
    m = spec.meshes[0]
    floor.load_raw(m.vertices, m.faces, m.uvs, m.face_uvs)
    sc.add_Mesh(floor, "tex", None)
    sc.add_Mesh(os.path.join(scenes.DATA, "cbox_smallbox.obj"), psdr.Matrix4fC(np.eye(4, dtype=np.float32).tolist()), "cat", None)
    sc.add_EnvironmentMap(psdr.EnvironmentMap(rad))
    sc.configure()
    sc.configure([0])
    integ = psdr.PathTracer(6)
    from psdr_jit_amd import cabi
    record_bytes = lambda: int(cabi.lib().psdr_hip_scene_adjoint_record_bytes(sc._hip_handle()))
    assert record_bytes() == 0          # a fresh scene: no global records yet
    w = Slot(torch, _weights(32 * 32, seed=4))
    v_rad = torch.tensor(rng.standard_normal(env0.shape).astype(np.float32))
    v_tex = torch.tensor(rng.standard_normal(tuple(tex.shape)).astype(np.float32))

    def first_backward():
        img = integ.renderD(sc, 0, seed=5)
        img.backward(w.buf)
        return torch.stack([(rad.grad * v_rad).sum(), (tex.grad * v_tex).sum()])
    got = run_on_stream(torch, streams[0], form, [w], first_backward, lambda g: g.cpu().numpy().astype(np.float64), returns_early=False)
    assert record_bytes() > 0          # plan.rec_in_lds was false: the call allocated and cleared the global records, under S
    img = integ.renderD(sc, 0, seed=5)
    wt = torch.from_numpy(w.true_np).to(img.device)
    want = np.array([float((psdr.forward_grad(img, rad, direction=v_rad) * wt).sum()), float((psdr.forward_grad(img, tex, direction=v_tex) * wt).sum())])
    print("deep paths, delay on %s: <J^T w, v> %s, forward mode %s" % (form, got, want))
    for k in range(2):
        assert abs(want[k]) > 1e-4 and abs(got[k] - want[k]) < 3e-3 * max(1.0, abs(want[k])), (k, got[k], want[k])


# ---------------------------------------------------------------------------------------------------------------------------
# 3. guiding
@pytest.mark.parametrize("form", FORMS)
def test_guiding_build(env, orc, streams, form):
    """psdr_hip_guiding_build with the stream of S: the cell masses against the oracle's (it synchronises inside: no self-check)"""
    torch, psdr, cabi = env
    spec = scenes.cbox_scene(32, 32, 2, 0, 4)
    sc = product.build_scene(spec)
    reso = [8, 4, 4, 4]
    want = orc.OracleScene(spec, [0]).guiding_build(0, reso, nrounds=2, seed=5).mass()
    L = cabi.lib()

    def build():
        h = C.c_void_p()
        cabi.check(L.psdr_hip_guiding_build(C.c_void_p(sc._hip_handle()), 0, 1, (C.c_int32 * 4)(*reso), 2, 5, C.byref(h), C.c_void_p(_ptr(torch))))
        mass = np.zeros(int(L.psdr_hip_guiding_num_cells(h)), np.float32)
        cabi.check(L.psdr_hip_guiding_mass(h, mass.ctypes.data_as(C.c_void_p), C.c_int32(mass.size)))
        cabi.check(L.psdr_hip_guiding_destroy(h))
        return mass
    for _ in range(2):          # (the second build meets the first one's freed allocation, full of the first one's masses, not fresh pages)
        mass = run_on_stream(torch, streams[0], form, [], build, lambda m: m, returns_early=False)
        assert mass.shape == want.shape and np.abs(want).max() > 0 and product.rel_l2(mass, want) < TOL


# ---------------------------------------------------------------------------------------------------------------------------
# 4. ray batches
N_RAYS = 4096


def _rays(seed):
    rng = np.random.default_rng(seed)
    o = rng.uniform([20, 20, 20], [530, 530, 540], size=(N_RAYS, 3)).astype(np.float32)
    d = rng.normal(size=(N_RAYS, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o, d


@pytest.mark.parametrize("form", FORMS)
def test_trace_and_intersect(env, orc, streams, form):
    """origins and directions produced behind the delay over other valid rays: psdr_hip_trace / _trace_pairs bit-equal to the oracle
    (test_gpu_parity.py::test_trace_matches_oracle); Scene.unit_ray_intersect valid where the oracle hits, its record the default stream's bit for bit"""
    torch, psdr, cabi = env
    S = streams[0]
    spec = scenes.cbox_scene(32, 32, 1, 0, 0)
    sc = product.build_scene(spec)
    ref = orc.OracleScene(spec, [0])
    o_np, d_np = _rays(3)
    o, d = Slot(torch, o_np), Slot(torch, d_np)
    wtri, wuv, wt = ref.trace(o_np, d_np, use_bvh=False)
    dtri = ref.trace(sc_.decoy_of(o_np), sc_.decoy_of(d_np), use_bvh=False)[0]
    hit = wtri >= 0
    assert hit.mean() > 0.5 and (dtri != wtri).mean() > 0.5          # (the decoy rays hit other triangles)
    L, h = cabi.lib(), sc._hip_handle()
    for fn, n in ((L.psdr_hip_trace, N_RAYS), (L.psdr_hip_trace_pairs, N_RAYS - 1)):
        def trace():
            tri = torch.full((N_RAYS,), -7, dtype=torch.int32, device="cuda")
            uv = torch.zeros((N_RAYS, 2), dtype=torch.float32, device="cuda")
            t = torch.zeros(N_RAYS, dtype=torch.float32, device="cuda")
            cabi.check(fn(h, n, o.buf.data_ptr(), d.buf.data_ptr(), tri.data_ptr(), uv.data_ptr(), t.data_ptr(), _ptr(torch)))
            return tri, uv, t
        tri, uv, t = run_on_stream(torch, S, form, [o, d], trace, lambda r: _cpu(*r))
        assert np.array_equal(tri[:n], wtri[:n]) and np.all(tri[n:] == -7)
        assert np.array_equal(uv[:n][hit[:n]], wuv[:n][hit[:n]]) and np.array_equal(t[:n][hit[:n]], wt[:n][hit[:n]])
    # Scene.unit_ray_intersect
    members = lambda its: [its.is_valid().to(torch.float32), its.t, its.p, its.n, its.uv, its.wi]
    got = run_on_stream(torch, S, form, [o, d], lambda: members(sc.unit_ray_intersect(psdr.RayC(o.buf, d.buf))), lambda r: _cpu(*r))
    base = run_plain(torch, [o, d], lambda: members(sc.unit_ray_intersect(psdr.RayC(o.buf, d.buf))), lambda r: _cpu(*r))
    assert np.array_equal(got[0] > 0, hit) and np.abs(got[1][hit]).max() > 0
    assert all(np.array_equal(a, b) for a, b in zip(got, base))


@pytest.mark.parametrize("form", FORMS)
def test_intersect_ad_forward_and_adjoint(env, orc, streams, form):
    """Scene.unit_ray_intersectAD under S: the record equals unit_ray_intersect's hits, and the adjoints of o and d - one thread per ray writes its own rows, no
    atomics - are the default stream's bit for bit; the adjoint of the rays' records g is produced behind the delay as well"""
    torch, psdr, _ = env
    S = streams[0]
    sc = product.build_scene(scenes.cbox_scene(32, 32, 1, 0, 0))
    o_np, d_np = _rays(4)
    o, d = Slot(torch, o_np), Slot(torch, d_np)
    g = Slot(torch, np.random.default_rng(6).standard_normal((N_RAYS, 3)).astype(np.float32))

    def run():
        oo, dd = o.buf.clone().requires_grad_(), d.buf.clone().requires_grad_()
        its = sc.unit_ray_intersectAD(psdr.RayD(oo, dd))
        its.p.backward(g.buf)
        return its.is_valid().to(torch.float32), its.t.detach(), its.p.detach(), oo.grad, dd.grad
    got = run_on_stream(torch, S, form, [o, d, g], run, lambda r: _cpu(*r), returns_early=False)          # (the chain to the leaves reads buffers back: it may synchronise)
    base = run_plain(torch, [o, d, g], run, lambda r: _cpu(*r))
    plain = sc.unit_ray_intersect(psdr.RayC(torch.from_numpy(o_np).cuda(), torch.from_numpy(d_np).cuda()))
    valid = plain.is_valid().cpu().numpy()
    assert valid.mean() > 0.5 and np.array_equal(got[0] > 0, valid)
    assert np.abs(got[3]).max() > 0 and np.abs(got[4]).max() > 0
    assert all(np.array_equal(a, b) for a, b in zip(got, base))


@pytest.mark.parametrize("form", FORMS)
def test_env_sample_and_pdf(env, orc, streams, form):
    """psdr_hip_env_sample / _env_pdf: bit-equal to the oracle, as in test_gpu_envmap.py; reference points and samples produced behind the delay"""
    torch, psdr, cabi = env
    spec = scenes.envmap_scene(32, 32, 1, 0, 0, param=None)
    sc = product.build_scene(spec)
    ref = orc.OracleScene(spec, [0])
    rng = np.random.default_rng(9)
    p_np = rng.uniform([0, 0, 0], [550, 300, 550], size=(N_RAYS, 3)).astype(np.float32)
    s_np = rng.random((N_RAYS, 2)).astype(np.float32)
    p, s2 = Slot(torch, p_np), Slot(torch, s_np)
    wp, wn, wpdf = ref.env_sample(p_np, s_np)
    L, h = cabi.lib(), sc._hip_handle()

    def sample():
        op, on = torch.zeros((N_RAYS, 3), device="cuda"), torch.zeros((N_RAYS, 3), device="cuda")
        opdf = torch.zeros(N_RAYS, device="cuda")
        cabi.check(L.psdr_hip_env_sample(h, N_RAYS, p.buf.data_ptr(), s2.buf.data_ptr(), op.data_ptr(), on.data_ptr(), opdf.data_ptr(), _ptr(torch)))
        return op, on, opdf
    op, on, opdf = run_on_stream(torch, streams[0], form, [p, s2], sample, lambda r: _cpu(*r))
    assert np.array_equal(op, wp) and np.array_equal(on, wn) and np.array_equal(opdf, wpdf)
    q, nn = Slot(torch, wp), Slot(torch, wn)

    def pdf():
        out = torch.zeros(N_RAYS, device="cuda")
        cabi.check(L.psdr_hip_env_pdf(h, N_RAYS, p.buf.data_ptr(), q.buf.data_ptr(), nn.buf.data_ptr(), out.data_ptr(), _ptr(torch)))
        return out
    got = run_on_stream(torch, streams[0], form, [p, q, nn], pdf, lambda t: t.cpu().numpy())
    assert np.array_equal(got, ref.env_pdf(p_np, wp, wn))


# ---------------------------------------------------------------------------------------------------------------------------
# 5. two streams, one scene
def test_two_streams_share_one_scene(env, orc, streams):
    """A renderD on A behind a delay, at once a renderD with another seed on B: both use the scene's queue ring, counters, traversal-stack tail and fork streams, and
    ScratchGuard makes B wait for A.  Then a backward on A followed by a forward on B.  Every result against its serial counterpart, at the bounds between two runs of
    the same samples."""
    torch, psdr, _ = env
    A, B = streams
    spec, sc, _ref, _want = _scene(env, orc, "bvh")
    integ = psdr.PathTracer(DEPTH)
    serial = {seed: run_plain(torch, [], lambda: psdr.render_d_fwd(integ, sc, 0, seed=seed), lambda o: _cpu(*o)) for seed in (31, 32)}
    torch.cuda.synchronize()
    with torch.cuda.stream(A):
        ev = sc_.delay(torch)
        a = psdr.render_d_fwd(integ, sc, 0, seed=31)
    with torch.cuda.stream(B):
        b = psdr.render_d_fwd(integ, sc, 0, seed=32)
        pending = not ev.query()
        b = _cpu(*b)
    with torch.cuda.stream(A):
        a = _cpu(*a)
    torch.cuda.synchronize()
    assert pending
    for got, want in ((a, serial[31]), (b, serial[32])):
        assert np.abs(want[1]).max() > 0 and product.rel_l2(got[0], want[0]) < TOL_IMAGE and product.rel_l2(got[1], want[1]) < TOL_DERIVATIVE
    assert product.rel_l2(a[1], b[1]) > 100 * TOL_DERIVATIVE          # (the two calls are told apart)
    # a backward on A, then a forward on B (the scene whose Mesh[0] translation is a leaf: its forward derivative has no tangent installed, the image is compared)
    spec, sc, P = _leaf_scene(env, "bvh")
    serial32 = run_plain(torch, [], lambda: psdr.render_d_fwd(integ, sc, 0, seed=32), lambda o: _cpu(*o))
    w = Slot(torch, _weights(spec.width * spec.height))
    base = float(run_plain(torch, [w], lambda: _backward(psdr, integ, sc, P, w.buf, 5), lambda g: g.cpu()))
    w.reset()
    torch.cuda.synchronize()
    with torch.cuda.stream(A):
        sc_.delay(torch)
        w.produce()
        grad = _backward(psdr, integ, sc, P, w.buf, 5)
    with torch.cuda.stream(B):
        b = _cpu(*psdr.render_d_fwd(integ, sc, 0, seed=32))
    with torch.cuda.stream(A):
        grad = float(grad.cpu())
    torch.cuda.synchronize()
    _, wd = orc.OracleScene(spec, [0]).render_d(max_depth=DEPTH, seeds=(5, 5, 5))
    want = float((wd.astype(np.float64) * w.true_np).sum())
    print("backward on A %.9g, default stream %.9g, oracle %.9g" % (grad, base, want))
    assert abs(grad - want) < 2e-3 * max(1.0, abs(want))
    assert abs(grad - base) < 2e-3 * max(1.0, abs(base))
    assert np.abs(serial32[0]).max() > 0 and product.rel_l2(b[0], serial32[0]) < TOL_IMAGE and np.array_equal(b[1] != 0, serial32[1] != 0)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. configure() between streams
def test_configure_waits_for_the_pending_render(env, orc, streams):
    """A render on A behind a delay; Mesh[0] moves and configure([0]) runs while that render is pending: the pending image is the OLD state's, a render on B afterwards the
    NEW state's - both against freshly built scenes, as test_gpu_configure.py::test_refit_keeps_the_hits_bit_equal judges a refitted scene.  (configure() waits for the
    scene's last call: it synchronises, the self-check is made before it.)"""
    torch, psdr, _ = env
    A, B = streams
    spec = SCENES["bvh"]()
    sc = product.build_scene(spec)
    integ = psdr.PathTracer(DEPTH)
    v0 = np.asarray(spec.meshes[0].vertices, np.float32).copy()
    v1 = (v0 * np.float32([1.0, 0.8, 1.0]) + np.float32([12.0, -3.0, 7.0])).astype(np.float32)
    old = integ.renderC(product.build_scene(spec), 0, seed=3).cpu().numpy()
    torch.cuda.synchronize()
    with torch.cuda.stream(A):
        ev = sc_.delay(torch)
        pending_img = integ.renderC(sc, 0, seed=3)
        pending = not ev.query()
        sc.param_map["Mesh[0]"]._set("vertex_positions", v1, np.zeros_like(v1))
        sc.configure([0])
        pending_img = pending_img.cpu().numpy()
    with torch.cuda.stream(B):
        new_img = integ.renderC(sc, 0, seed=3).cpu().numpy()
    torch.cuda.synchronize()
    assert pending
    spec.meshes[0].vertices = v1
    new = integ.renderC(product.build_scene(spec), 0, seed=3).cpu().numpy()
    assert product.rel_l2(old, new) > 1e-2          # (the two states are told apart)
    assert product.rel_l2(pending_img, old) < 1e-6 and product.rel_l2(new_img, new) < 1e-6


# ---------------------------------------------------------------------------------------------------------------------------
# 7. handles across streams
W7, H7, L7, C7, G7 = 67, 35, 3, 3, 8


def _make_under(torch, stream, slots, others, make, poison=None):
    """a handle constructed under `stream` with its device inputs produced behind a delay on it.  Nothing is synchronised afterwards: the test applies the handle at once
    under another stream (run_on_stream(..., follows_at_once=True)), which is only right because every create returns with the handle usable on any stream - it waits for
    its stream, so no self-check here.  `others`: the slots of that first apply, reset here.  The delay is twice the usual one, so that it outlasts the delay the first
    apply queues on its own stream.  poison: makes a handle of the same size from the DECOY inputs, which is dropped at once: the block the allocator hands to make()
    then holds a valid but wrong operator, not - by chance - the right one an earlier test left there."""
    for s in list(slots) + list(others):
        s.reset()
    if poison is not None:
        handle = poison()
        torch.cuda.synchronize()
        del handle
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        sc_.delay(torch)
        sc_.delay(torch)
        for s in slots:
            s.produce()
        return make()


@pytest.mark.parametrize("form", FORMS)
def test_denoiser_made_on_one_stream_applied_on_another(env, streams, form):
    import test_denoise_cpu as dcpu
    import test_gpu_denoise as tgd
    torch, psdr, _ = env
    A, B = streams
    rng = np.random.default_rng(71)
    g_np = dcpu._guides(rng, W7, H7, G7)
    x_np, y_np = tgd._image(rng, W7 * H7, C7), tgd._image(rng, W7 * H7, C7)
    g, x, y = Slot(torch, g_np), Slot(torch, x_np), Slot(torch, y_np)
    plain = psdr.Denoiser(torch.from_numpy(g_np), W7, H7, levels=L7)
    base = run_plain(torch, [x], lambda: plain(x.buf), lambda t: t.cpu().numpy())
    base_t = run_plain(torch, [y], lambda: plain.transpose(y.buf), lambda t: t.cpu().numpy())
    den = _make_under(torch, A, [g], [x], lambda: psdr.Denoiser(g.buf, W7, H7, levels=L7), poison=lambda: psdr.Denoiser(g._decoy, W7, H7, levels=L7))
    g.reset()          # (the guides are the caller's again after the create: overwriting them does not reach the handle)
    got = run_on_stream(torch, B, form, [x], lambda: den(x.buf), lambda t: t.cpu().numpy(), follows_at_once=True)
    got_t = run_on_stream(torch, B, form, [y], lambda: den.transpose(y.buf), lambda t: t.cpu().numpy())
    want, want_t = denoise_ref.apply(x_np, g_np, W7, H7, L7), denoise_ref.apply_adj(y_np, g_np, W7, H7, L7)
    bound = L7 * tgd.k_of(G7) * U * np.abs(x_np).max()
    assert np.all(np.abs(got.astype(np.float64) - want) <= bound)
    assert np.all(np.abs(got_t.astype(np.float64) - want_t) <= tgd.adjoint_bound(y_np, g_np, W7, H7, L7, G7))
    assert np.abs(denoise_ref.apply(x_np, sc_.decoy_of(g_np), W7, H7, L7) - want).max() > 10 * bound          # (a handle made from the decoy guides is outside the bound)
    assert np.array_equal(got, base) and np.array_equal(got_t, base_t)

    def autograd():
        leaf = x.buf.clone().requires_grad_()
        den(leaf).backward(y.buf)
        return leaf.grad
    x.produce()
    assert np.array_equal(run_on_stream(torch, B, form, [y], autograd, lambda t: t.cpu().numpy(), returns_early=False), got_t)


@pytest.mark.parametrize("form", FORMS)
def test_variance_denoiser_made_on_one_stream_applied_on_another(env, streams, form):
    import test_denoise_cpu as dcpu
    import test_gpu_vdenoise as tgv
    import test_vdenoise_cpu as vcpu
    torch, psdr, _ = env
    A, B = streams
    rng = np.random.default_rng(72)
    g_np = dcpu._guides(rng, W7, H7, G7)
    x_np, v_np = vcpu._inputs(rng, W7, H7, C7)
    u_np = tgv.dcpu_image(rng, W7 * H7, C7)
    g, x, v, u = Slot(torch, g_np), Slot(torch, x_np), Slot(torch, v_np), Slot(torch, u_np)
    make = lambda guides: psdr.VarianceDenoiser(guides, W7, H7, levels=L7, sigma_l=2.0, eps=tgv.EPS)
    plain = make(torch.from_numpy(g_np))
    base = run_plain(torch, [x, v, u], lambda: (plain(x.buf, v.buf), plain.variance, plain.frozen(u.buf), plain.frozen_transpose(u.buf)), lambda o: _cpu(*o))
    den = _make_under(torch, A, [g], [x, v], lambda: make(g.buf), poison=lambda: make(g._decoy))
    g.reset()
    got, got_v = run_on_stream(torch, B, form, [x, v], lambda: (den(x.buf, v.buf), den.variance), lambda o: _cpu(*o), follows_at_once=True)
    want, want_v, tol, tol_v = tgv.reference_tolerance(x_np, v_np, g_np, W7, H7, L7)
    assert np.all(np.abs(got.astype(np.float64) - want) <= tol) and np.all(np.abs(got_v.astype(np.float64) - want_v) <= tol_v)
    rec = run_on_stream(torch, B, form, [], lambda: den.record(), lambda t: t.cpu().numpy())
    record = vdenoise_ref.record_planes(rec, W7, H7)
    fz = run_on_stream(torch, B, form, [u], lambda: den.frozen(u.buf), lambda t: t.cpu().numpy())
    fz_t = run_on_stream(torch, B, form, [u], lambda: den.frozen_transpose(u.buf), lambda t: t.cpu().numpy())
    assert np.all(np.abs(fz.astype(np.float64) - vdenoise_ref.frozen(u_np, g_np, record, W7, H7, tgv.K_L, tgv.EPS)) <= L7 * tgv.k_of(G7) * U * np.abs(u_np).max())
    assert np.all(np.abs(fz_t.astype(np.float64) - vdenoise_ref.frozen_adj(u_np, g_np, record, W7, H7, tgv.K_L, tgv.EPS)) <= tgv.adjoint_bound(u_np, g_np, record, W7, H7, G7))
    assert all(np.array_equal(a, b) for a, b in zip((got, got_v, fz, fz_t), base))

    def autograd():
        leaf = x.buf.clone().requires_grad_()
        den(leaf, v.buf).backward(u.buf)
        return leaf.grad
    x.produce(); v.produce()
    assert np.array_equal(run_on_stream(torch, B, form, [u], autograd, lambda t: t.cpu().numpy(), returns_early=False), fz_t)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["tetrahedron", "fan"])
def test_subdivision_made_on_one_stream_applied_on_another(env, streams, name, form):
    import test_gpu_subdiv as tgs
    torch, psdr, _ = env
    A, B = streams
    faces, n, _levels = tgs._mesh(name)
    S64 = subdiv_ref.reference_chain(name, faces, n, "loop", 1)[0][0]
    plain = psdr.Subdivision(faces, n, levels=1, scheme="loop")
    rng = np.random.default_rng(26)
    x_np = rng.standard_normal((n, 3)).astype(np.float32)
    y_np = rng.standard_normal((plain.num_vertices_out, 3)).astype(np.float32)
    x, y = Slot(torch, x_np), Slot(torch, y_np)
    base = run_plain(torch, [x], lambda: plain.refine(x.buf), lambda t: t.cpu().numpy())
    base_t = run_plain(torch, [y], lambda: plain.restrict(y.buf), lambda t: t.cpu().numpy())
    sub = _make_under(torch, A, [], [x], lambda: psdr.Subdivision(faces, n, levels=1, scheme="loop"))
    got = run_on_stream(torch, B, form, [x], lambda: sub.refine(x.buf), lambda t: t.cpu().numpy(), follows_at_once=True)
    got_t = run_on_stream(torch, B, form, [y], lambda: sub.restrict(y.buf), lambda t: t.cpu().numpy())
    for g, inp, transpose in ((got, x_np, False), (got_t, y_np, True)):
        want, bound = tgs._bounds(S64, inp, transpose)
        tgs._check(g, want, bound, "%s, delay on %s, transpose %s" % (name, form, transpose))
    assert np.array_equal(got, base) and np.array_equal(got_t, base_t)

    def autograd():
        leaf = x.buf.clone().requires_grad_()
        (sub.refine(leaf) * y.buf).sum().backward()
        return leaf.grad
    x.produce()
    assert np.array_equal(run_on_stream(torch, B, form, [y], autograd, lambda t: t.cpu().numpy(), returns_early=False), got_t)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["tetrahedron", "fan"])
def test_preconditioner_made_on_one_stream_applied_on_another(env, streams, name, form):
    import test_gpu_precond as tgp
    torch, psdr, _ = env
    A, B = streams
    faces, n, lam = tgp._mesh(psdr, name)
    M = tgp._matrix(faces, n, lam)
    plain = psdr.LaplacianPreconditioner(faces, n, lambda_=lam, rtol=tgp.RTOL)
    b_np = np.random.default_rng(5).standard_normal((n, 3)).astype(np.float32)
    b = Slot(torch, b_np)
    base_y = run_plain(torch, [b], lambda: plain.to_differential(b.buf), lambda t: t.cpu().numpy())
    base_x = run_plain(torch, [b], lambda: plain.from_differential(b.buf), lambda t: t.cpu().numpy())
    pre = _make_under(torch, A, [], [b], lambda: psdr.LaplacianPreconditioner(faces, n, lambda_=lam, rtol=tgp.RTOL))
    # the product returns without synchronising; the solve reads its residuals back (it synchronises inside: no self-check)
    y = run_on_stream(torch, B, form, [b], lambda: pre.to_differential(b.buf), lambda t: t.cpu().numpy(), follows_at_once=True)
    assert np.all(np.abs(y.astype(np.float64) - M @ b_np.astype(np.float64)) <= tgp._apply_bound(pre, lam, b_np))
    x = run_on_stream(torch, B, form, [b], lambda: pre.from_differential(b.buf), lambda t: t.cpu().numpy(), returns_early=False)
    assert pre.last_solve["converged"]
    tgp._check_solution(x, M, b_np, "%s, delay on %s" % (name, form))
    assert np.array_equal(y, base_y) and np.array_equal(x, base_x)

    def autograd():
        leaf = torch.ones((n, 3), device="cuda").requires_grad_()
        (pre.from_differential(leaf) * b.buf).sum().backward()          # the backward of the solve is a solve of the adjoint b
        return leaf.grad
    assert np.array_equal(run_on_stream(torch, B, form, [b], autograd, lambda t: t.cpu().numpy(), returns_early=False), x)


# ---------------------------------------------------------------------------------------------------------------------------
# 8. adaptive sampling
N8 = 1025          # the smallest size of test_gpu_adaptive.py that spans two tiles


@pytest.mark.parametrize("form", FORMS)
def test_adaptive_plan_and_fold(env, streams, form):
    import test_adaptive_cpu as rule
    import test_gpu_adaptive as tga
    torch, psdr, _ = env
    S = streams[0]
    rng = np.random.default_rng(1000 + N8)
    w_np = np.ascontiguousarray(rule.weight_maps(N8, rng)["random"], dtype=np.float32)
    budget = 7 * N8 + 3
    counts, offsets, _, _ = rule.allocate(w_np, budget, 2)
    w = Slot(torch, w_np)
    got = run_on_stream(torch, S, form, [w], lambda: psdr.PixelPlan.from_weights(w.buf, budget, 2), lambda p: _cpu(p.counts, p.offsets, p.pix))
    assert np.array_equal(got[0], counts) and np.array_equal(got[1], offsets) and np.array_equal(got[2], np.repeat(np.arange(N8), counts))
    assert not np.array_equal(rule.allocate(sc_.decoy_of(w_np), budget, 2)[0], counts)
    # the fold and its transpose over offsets produced behind the delay; the decoy is another monotone list with the same total (the counts in another order)
    d_counts = sc_.decoy_of(counts)
    d_offsets = np.concatenate([[0], np.cumsum(d_counts)]).astype(np.int32)
    assert d_offsets[-1] == offsets[-1] == budget
    off = Slot(torch, offsets.astype(np.int32), d_offsets)
    pix = np.repeat(np.arange(N8), counts).astype(np.int32)
    plan = psdr.PixelPlan(torch.from_numpy(counts.astype(np.int32)).cuda(), off.buf, torch.from_numpy(pix).cuda(), N8, budget)
    rows_np = (rng.standard_normal((budget, 3)) * 10.0 ** rng.uniform(-2, 2, (budget, 1))).astype(np.float32)
    base_np = rng.standard_normal((N8, 3)).astype(np.float32)
    y_np = rng.standard_normal((N8, 3)).astype(np.float32)
    rows, base, y = Slot(torch, rows_np), Slot(torch, base_np), Slot(torch, y_np)
    out = run_on_stream(torch, S, form, [off, rows, base], lambda: plan.merge(rows.buf, 4.0, base.buf, 8.0), lambda t: t.cpu().numpy())
    want, terms = tga._fold64(counts, pix, rows_np, 4.0, base_np, 8.0, 0)
    assert np.all(np.abs(out.astype(np.float64) - want) <= (counts[:, None] + 2) * U * terms)
    assert np.array_equal(out, run_plain(torch, [off, rows, base], lambda: plan.merge(rows.buf, 4.0, base.buf, 8.0), lambda t: t.cpu().numpy()))

    def transpose():
        r, b = rows.buf.clone().requires_grad_(), base.buf.clone().requires_grad_()
        plan.merge(r, 4.0, b, 8.0).backward(y.buf)
        return r.grad, b.grad
    rows.produce(); base.produce()
    d_rows, d_base = run_on_stream(torch, S, form, [off, y], transpose, lambda o: _cpu(*o), returns_early=False)
    n_tot = 8.0 + 4.0 * counts.astype(np.float64)
    want_rows, want_base = (4.0 / n_tot)[pix, None] * y_np[pix].astype(np.float64), (8.0 / n_tot)[:, None] * y_np.astype(np.float64)
    assert np.all(np.abs(d_rows - want_rows) <= 2 * U * np.abs(want_rows)) and np.all(np.abs(d_base - want_base) <= 2 * U * np.abs(want_base))
    assert all(np.array_equal(a, b) for a, b in zip((d_rows, d_base), run_plain(torch, [off, y], transpose, lambda o: _cpu(*o))))
