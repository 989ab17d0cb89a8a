"""Every render path through sensors other than Sensor[0].

Multi-view optimisation adds several sensors, calls configure([ids]) and renders each view in every step; a good deal of device and host state is indexed by the
sensor (SensorDev and its primary-edge section of the blob, the live-pixel mask, the guiding grid, the slot table of batch edge terms, the sensor id renderD records for
backward(), chain.native_geometry_grads, the leaves of Sensor[k], configure's active list, the incremental scene update).  If one of them read Sensor[0]'s entry while
another sensor was rendered, the image would look plausible and every test that passes sensor id 0 would still pass.  The scenes are the three-sensor scenes of
tests/sensor_cases.py; tests/test_sensors_cpu.py asserts on the oracle that their sensors see different things, so an answer for the wrong sensor is far outside every
bound used here.

Bounds, none of them taken from what this code gives:
   TOL = 1e-3 rel-L2 against the oracle (test_gpu_parity.py, BASELINE north_star; observed ~1e-7);
   2e-6 of the largest entry where two launches add the same samples in another order of float atomics (test_gpu_configs.py, skip_static_edges);
   1e-6 / 1e-5 rel-L2 where shards add up to the frame (test_gpu_parity.py::test_shards_sum_to_full_frame);
   2e-3 max(1, |want|) for reverse mode against forward mode and against the oracle, 3e-3 for camera poses (test_gpu_api.py, test_gpu_envmap.py);
   1e-6 rel-L2 against a scene built from scratch in the same state (test_gpu_configure.py, test_gpu_device_edges.py);
   exact equality where the oracle's derivative is exactly zero and where nothing a sensor reads has changed."""
import ctypes as C

import numpy as np
import pytest

import product
import scenes
import sensor_cases as cases

pytestmark = pytest.mark.gpu
TOL = 1e-3       # BASELINE north_star: gradient L2 error < 1e-3; observed ~1e-7
ATOMIC_TOL = 2e-6
FRESH_TOL = 1e-6
DEPTH = cases.DEPTH
N = cases.W * cases.H
RESO = [40, 4, 4, 16]


@pytest.fixture(scope="module")
def psdr():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists)")
    import __graft_entry__
    __graft_entry__.build()
    import psdr_jit_amd
    return psdr_jit_amd


@pytest.fixture(scope="module")
def three(psdr, orc):
    """family -> (spec, product scene, oracle scene) with all three sensors active, built once; for the tests that only render"""
    cache = {}

    def get(family):
        if family not in cache:
            spec = cases.family_spec(family)
            cache[family] = (spec, product.build_scene(spec, active=(0, 1, 2)), orc.OracleScene(spec, [0, 1, 2]))
        return cache[family]
    return get


def _check_terms(psdr, orc, sc, ref, k, what, integ=None, depth=DEPTH, seed=5, guiding=None, terms_list=None):
    """render_d_fwd through sensor k, term by term, against the oracle's sensor k; where the oracle's derivative is exactly zero so is the product's"""
    integ = integ if integ is not None else psdr.PathTracer(depth)
    for terms in terms_list or (orc.TERM_INTERIOR, orc.TERM_PRIMARY, orc.TERM_SECONDARY, orc.TERM_ALL):
        img, dimg = psdr.render_d_fwd(integ, sc, k, seed=seed, terms=terms)
        wimg, wd = ref.render_d(sensor=k, max_depth=depth, seeds=(seed, seed, seed), terms=terms, guiding=guiding)
        if terms & orc.TERM_INTERIOR:
            assert product.rel_l2(img.cpu().numpy(), wimg) < TOL, (what, k, terms)
        else:
            assert float(img.abs().max()) == 0.0, (what, k, terms)          # edge terms have zero primal
        if np.abs(wd).max() > 0:
            assert product.rel_l2(dimg.cpu().numpy(), wd) < TOL, (what, k, terms)
        else:
            assert float(dimg.abs().max()) == 0.0, (what, k, terms)


# --------------------------------------------------------------------------------------------------------------------------- a. forward, per term, per scene class
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("family", cases.FAMILIES)
def test_forward_terms_through_sensor_k(psdr, orc, three, family, k):
    spec, sc, ref = three(family)
    c = psdr.PathTracer(DEPTH).renderC(sc, k, seed=7).cpu().numpy()
    want = ref.render_c(sensor=k, max_depth=DEPTH, seed=7)
    assert np.isfinite(c).all() and c.shape == want.shape and product.rel_l2(c, want) < TOL
    _check_terms(psdr, orc, sc, ref, k, family)


# --------------------------------------------------------------------------------------------------------------------------- b. camera tangents
@pytest.mark.parametrize("camera,other", [(1, 0), (0, 1)])
@pytest.mark.parametrize("family", cases.FAMILIES)
def test_a_camera_tangent_reaches_its_own_sensor_only(psdr, orc, family, camera, other):
    spec = cases.camera_tangent_spec(family, camera)
    sc = product.build_scene(spec, active=(0, 1, 2))
    ref = orc.OracleScene(spec, [0, 1, 2])
    for terms in (orc.TERM_INTERIOR, orc.TERM_PRIMARY, orc.TERM_SECONDARY):
        assert np.abs(ref.render_d(sensor=camera, max_depth=DEPTH, seeds=(5, 5, 5), terms=terms)[1]).max() > 0
        _, d_other = psdr.render_d_fwd(psdr.PathTracer(DEPTH), sc, other, seed=5, terms=terms)
        assert float(d_other.abs().max()) == 0.0, (family, other, terms)
    _check_terms(psdr, orc, sc, ref, camera, family)
    _check_terms(psdr, orc, sc, ref, other, family, terms_list=(orc.TERM_ALL,))


# --------------------------------------------------------------------------------------------------------------------------- c. active subsets
@pytest.mark.parametrize("family", ["cbox", "envmap"])
def test_active_subsets(psdr, orc, family):
    spec = cases.family_spec(family)
    sc = product.build_scene(spec, active=(1,))
    ref = orc.OracleScene(spec, [1])
    assert ref.num_primary_edges(0) == 0 and ref.num_primary_edges(1) > 0
    for k in (1, 0):            # sensor 0 is not active: interior and secondary terms as ever, no primary term
        _check_terms(psdr, orc, sc, ref, k, family + " [1]")
    assert len(np.asarray(sc.param_map["Sensor[0]"]._primary_edge_ids()).reshape(-1, 3)) == 0
    sc.configure([0, 2])
    ref = orc.OracleScene(spec, [0, 2])
    assert ref.num_primary_edges(1) == 0 and ref.num_primary_edges(0) > 0 and ref.num_primary_edges(2) > 0
    for k in (0, 2, 1):
        _check_terms(psdr, orc, sc, ref, k, family + " [0, 2]")
    sc.configure()              # the empty list: no sensor keeps primary edges
    ref = orc.OracleScene(spec, [])
    for k in (0, 1):
        assert ref.num_primary_edges(k) == 0
        _check_terms(psdr, orc, sc, ref, k, family + " []")


# --------------------------------------------------------------------------------------------------------------------------- d. through the C ABI
def _render_d_abi(torch, sc, **kw):
    from psdr_jit_amd import cabi
    buf = torch.empty((2, N, 3), dtype=torch.float32, device="cuda")
    a = cabi.make_args(sensor_id=1, max_depth=DEPTH, **kw)
    cabi.check(cabi.lib().psdr_hip_render_d_fwd(sc._hip_handle(), C.byref(a), buf[0].data_ptr(), buf[1].data_ptr(), None))
    return buf.cpu().numpy()


def test_c_abi_entry_points_with_sensor_id_1(psdr, orc, three):
    import torch
    from psdr_jit_amd import cabi
    L = cabi.lib()
    spec, sc, ref = three("cbox")
    # psdr_hip_li_lanes, under the bound of test_gpu_parity.py::test_lane_radiance_matches_oracle
    n = N * spec.spp
    out = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    a = cabi.make_args(sensor_id=1, max_depth=DEPTH, seeds=(5, 0, 0))
    cabi.check(L.psdr_hip_li_lanes(sc._hip_handle(), C.byref(a), 0, n, out.data_ptr(), None))
    got, want = out.cpu().numpy(), ref.li_lanes(0, n, sensor=1, max_depth=DEPTH, seed=5)
    scale = np.abs(want).max()
    bad = np.abs(got - want).max(axis=1) > 1e-4 * scale
    assert scale > 0 and bad.mean() < 2e-4, "fraction of lanes off by >1e-4: %g" % bad.mean()
    assert product.rel_l2(got[~bad], want[~bad]) < 1e-5
    # psdr_hip_render_c_counted gives the image of psdr_hip_render_c
    a = cabi.make_args(sensor_id=1, max_depth=DEPTH, seeds=(1, 0, 0))
    counted, plain, cnt = torch.empty((N, 3), dtype=torch.float32, device="cuda"), torch.empty((N, 3), dtype=torch.float32, device="cuda"), cabi.Counters()
    cabi.check(L.psdr_hip_render_c_counted(sc._hip_handle(), C.byref(a), counted.data_ptr(), C.byref(cnt), None))
    cabi.check(L.psdr_hip_render_c(sc._hip_handle(), C.byref(a), plain.data_ptr(), None))
    assert cnt.rays >= n and torch.allclose(counted, plain, rtol=1e-5, atol=1e-6)
    assert product.rel_l2(plain.cpu().numpy(), ref.render_c(sensor=1, max_depth=DEPTH, seed=1)) < TOL
    # skip_static_edges: the same image and derivative as without it, and as the oracle
    full = _render_d_abi(torch, sc, seeds=(4, 4, 4))
    skipped = _render_d_abi(torch, sc, seeds=(4, 4, 4), skip_static_edges=True)
    w0, w1 = ref.render_d(sensor=1, max_depth=DEPTH, seeds=(4, 4, 4))
    for buf in (full, skipped):
        assert product.rel_l2(buf[0], w0) < TOL and product.rel_l2(buf[1], w1) < TOL
    for k in (0, 1):
        assert np.abs(skipped[k] - full[k]).max() <= ATOMIC_TOL * np.abs(full[k]).max(), k
    # shards: one against the oracle's, three summing to the frame (test_gpu_parity.py::test_shards_sum_to_full_frame)
    one = _render_d_abi(torch, sc, seeds=(4, 4, 4), shard_rank=1, shard_count=3)
    s0, s1 = ref.render_d(sensor=1, max_depth=DEPTH, seeds=(4, 4, 4), shard_rank=1, shard_count=3)
    assert np.abs(s1).max() > 0 and product.rel_l2(one[0], s0) < TOL and product.rel_l2(one[1], s1) < TOL
    parts = one + _render_d_abi(torch, sc, seeds=(4, 4, 4), shard_rank=0, shard_count=3) + _render_d_abi(torch, sc, seeds=(4, 4, 4), shard_rank=2, shard_count=3)
    assert product.rel_l2(parts[0], full[0]) < 1e-6 and product.rel_l2(parts[1], full[1]) < 1e-5


# --------------------------------------------------------------------------------------------------------------------------- e. live-pixel mask
def _live_mask(sc, k):
    from psdr_jit_amd import cabi
    bits = np.zeros((N + 31) // 32, np.uint32)
    n_live = C.c_int64(0)
    cabi.check(cabi.lib().psdr_hip_scene_live_pixels(C.c_void_p(sc._hip_handle()), k, bits.ctypes.data, C.byref(n_live)))
    return bits, n_live.value


def _check_live_mask(sc, k, what):
    """the three assertions of test_gpu_parity.py::test_live_pixel_mask_is_conservative_and_exact, for sensor k -> the mask's words"""
    import torch
    from psdr_jit_amd import cabi
    bits, n_live = _live_mask(sc, k)
    live = ((bits[np.arange(N) >> 5] >> (np.arange(N) & 31).astype(np.uint32)) & 1).astype(bool)
    assert int(live.sum()) == n_live, (what, k)
    a = cabi.make_args(sensor_id=k, max_depth=0, seeds=(3, 3, 3), terms=1, field=0)          # the silhouette field: 1 where a camera ray of sensor k hits anything
    img = torch.zeros((N, 3), dtype=torch.float32, device="cuda")
    cabi.check(cabi.lib().psdr_hip_render_c(C.c_void_p(sc._hip_handle()), C.byref(a), img.data_ptr(), None))
    hit = img.cpu().numpy()[:, 0] > 0
    assert hit.sum() > 0 and not np.any(hit & ~live), (what, k, int((hit & ~live).sum()))
    assert live.sum() <= 2.5 * hit.sum() + 4 * (cases.W + cases.H), (what, k, int(live.sum()), int(hit.sum()))
    return bits


def test_live_pixel_mask_of_every_sensor(psdr, orc, three):
    spec, sc, ref = three("cbox")
    masks = [_check_live_mask(sc, k, "cbox") for k in range(3)]
    assert not np.array_equal(masks[0], masks[1]) and not np.array_equal(masks[1], masks[2])


# --------------------------------------------------------------------------------------------------------------------------- f. guiding
def test_guiding_grid_per_sensor(psdr, orc, three):
    spec, sc, ref = three("cbox")
    integ = psdr.PathTracer(DEPTH)
    sec = (orc.TERM_SECONDARY,)
    integ.preprocess_secondary_edges(sc, 1, RESO, 1, 5)
    g1 = ref.guiding_build(1, RESO, nrounds=1, seed=5, max_depth=DEPTH)
    mass = np.asarray(integ._guiding_mass(1)).reshape(-1)
    assert mass.shape == g1.mass().shape and product.rel_l2(mass, g1.mass()) < TOL
    _check_terms(psdr, orc, sc, ref, 1, "grid of sensor 1", integ=integ, seed=6, guiding=g1, terms_list=sec)
    _check_terms(psdr, orc, sc, ref, 0, "no grid for sensor 0", integ=integ, seed=6, terms_list=sec)
    # (the grid matters: the unguided term of sensor 1 is another estimate)
    _, unguided = ref.render_d(sensor=1, max_depth=DEPTH, seeds=(6, 6, 6), terms=orc.TERM_SECONDARY)
    _, guided = ref.render_d(sensor=1, max_depth=DEPTH, seeds=(6, 6, 6), terms=orc.TERM_SECONDARY, guiding=g1)
    assert product.rel_l2(guided, unguided) > 0.1
    integ.preprocess_secondary_edges(sc, 0, RESO, 1, 5)
    g0 = ref.guiding_build(0, RESO, nrounds=1, seed=5, max_depth=DEPTH)
    assert product.rel_l2(np.asarray(integ._guiding_mass(0)).reshape(-1), g0.mass()) < TOL
    assert product.rel_l2(np.asarray(integ._guiding_mass(1)).reshape(-1), g1.mass()) < TOL
    _check_terms(psdr, orc, sc, ref, 1, "both grids, sensor 1", integ=integ, seed=6, guiding=g1, terms_list=sec + (orc.TERM_ALL,))
    _check_terms(psdr, orc, sc, ref, 0, "both grids, sensor 0", integ=integ, seed=6, guiding=g0, terms_list=sec + (orc.TERM_ALL,))


# --------------------------------------------------------------------------------------------------------------------------- g. batch pixels
def test_batch_pixels_through_sensor_1(psdr, orc, three):
    """seven entries, one pixel twice; 981, 1090, 1050 lie on primary edges of sensor 1 and 981, 1090, 1130 carry its secondary term (none of them does for sensor 0)"""
    import torch
    spec, sc, ref = three("cbox")
    pix = np.array([981, 1090, 1050, 1130, 1090, 5, N - 1], dtype=np.int32)
    integ = psdr.PathTracer(DEPTH)
    img = integ.renderC(sc, 1, seed=3, batch_pix=torch.from_numpy(pix)).cpu().numpy()
    assert img.shape == (len(pix), 3) and product.rel_l2(img, ref.render_c(sensor=1, max_depth=DEPTH, seed=3, pix_ids=pix)) < TOL
    want_img, want_int = ref.render_d(sensor=1, max_depth=DEPTH, seeds=(21, 21, 21), pix_ids=pix)          # (a pixel list in the oracle: interior only)
    _, want_p = ref.render_d(sensor=1, max_depth=DEPTH, seeds=(21, 21, 21), terms=orc.TERM_PRIMARY)
    _, want_s = ref.render_d(sensor=1, max_depth=DEPTH, seeds=(21, 21, 21), terms=orc.TERM_SECONDARY)
    assert (np.abs(want_p[pix]).max(axis=1) > 0).sum() >= 4 and (np.abs(want_s[pix]).max(axis=1) > 0).sum() >= 4
    img, dimg = psdr.render_d_fwd(integ, sc, 1, seed=21, batch_pix=torch.from_numpy(pix), batch_edges=True)
    assert tuple(dimg.shape) == (len(pix), 3) and product.rel_l2(img.cpu().numpy(), want_img) < TOL
    assert product.rel_l2(dimg.cpu().numpy(), want_int + want_p[pix] + want_s[pix]) < TOL
    for term, want in ((orc.TERM_PRIMARY, want_p), (orc.TERM_SECONDARY, want_s)):
        _, d = psdr.render_d_fwd(integ, sc, 1, seed=21, batch_pix=torch.from_numpy(pix), batch_edges=True, terms=term)
        assert product.rel_l2(d.cpu().numpy(), want[pix]) < TOL, term
    # ... and through Integrator.renderD
    plain = integ.renderD(sc, 1, seed=21, batch_pix=torch.from_numpy(pix), batch_edges=True)
    assert product.rel_l2(plain.cpu().numpy(), want_img) < TOL


# --------------------------------------------------------------------------------------------------------------------------- h. other integrators
def test_direct_and_field_integrators_through_sensor_1(psdr, orc):
    spec = cases.family_spec("cbox")
    sc = product.build_scene(spec, active=(0, 1, 2))
    ref = orc.OracleScene(spec, [0, 1, 2])              # (its own: set_direct_mis / set_field change it)
    ref.set_direct_mis(1)
    integ = psdr.Direct(1)
    c = integ.renderC(sc, 1, seed=5).cpu().numpy()
    assert c.mean() > 0 and product.rel_l2(c, ref.render_c(sensor=1, max_depth=1, seed=5)) < TOL
    _check_terms(psdr, orc, sc, ref, 1, "Direct(1)", integ=integ, depth=1, seed=9)
    ref.set_direct_mis(-1)
    for name, obj in (("depth", -1), ("silhouette", 1)):
        integ = psdr.FieldExtractionIntegrator(name + (" %d" % obj if obj >= 0 else ""))
        ref.set_field(name, obj=obj)
        img, dimg = psdr.render_d_fwd(integ, sc, 1, seed=3)
        wimg, wd = ref.render_d(sensor=1, max_depth=0, seeds=(3, 3, 3))
        assert np.abs(wimg).max() > 0 and product.rel_l2(img.cpu().numpy(), wimg) < TOL, name
        assert np.abs(wd).max() > 0 and product.rel_l2(dimg.cpu().numpy(), wd) < TOL, name


# --------------------------------------------------------------------------------------------------------------------------- i, j. reverse mode
def _leafy_scene(psdr, family):
    """the family's scene with four leaves: P (Mesh[1] translated by 100 P along x), the albedo of Mesh[1]'s BSDF, and C0 / C1 (Sensor[0] / Sensor[1] translated by
    50 C along x) -> (scene, leaves, the oracle's spec of the same state with P's tangent)"""
    import torch
    spec = cases.family_spec(family, moving=False)
    bsdf = spec.bsdfs[spec.meshes[1].bsdf]
    bsdf.reflectance = (0.5, 0.4, 0.6)
    sc = product.build_scene(spec, active=(0, 1, 2))
    P, C0, C1 = (psdr.FloatD(0.).requires_grad_() for _ in range(3))
    albedo = torch.tensor([0.5, 0.4, 0.6], requires_grad=True)
    sc.param_map["BSDF[id=%s]" % bsdf.name].reflectance = albedo
    sc.param_map["Mesh[1]"].set_transform(psdr.Matrix4fD([[1., 0., 0., P * 100.], [0., 1., 0., 0.], [0., 0., 1., 0.], [0., 0., 0., 1.]]))
    shift = torch.zeros(4, 4); shift[0, 3] = 1.0
    for k, c in ((0, C0), (1, C1)):
        base = torch.tensor(np.asarray(spec.cameras[k].to_world_raw, np.float32))
        sc.param_map["Sensor[%d]" % k].to_world = psdr.Matrix4fD(base + shift * c * 50.)
    sc.configure([0, 1, 2])
    dT = np.zeros((4, 4), np.float32); dT[0, 3] = 100.0
    spec.meshes[1].d_to_world_left = dT
    return sc, {"P": P, "albedo": albedo, "C0": C0, "C1": C1}, spec


def _forward_values(psdr, img, w, leaves):
    import torch
    return {name: float((psdr.forward_grad(img, t, direction=torch.ones(3) if name == "albedo" else None) * w).sum()) for name, t in leaves.items()}


def _grad_values(leaves):
    return {name: (0.0 if t.grad is None else float(t.grad.sum())) for name, t in leaves.items()}


def _bound(name, want):
    return (3e-3 if name.startswith("C") else 2e-3) * max(1.0, abs(want))


@pytest.mark.parametrize("family", ["cbox", "sphere"])
def test_reverse_mode_through_sensor_1(psdr, orc, family):
    import torch
    sc, leaves, spec = _leafy_scene(psdr, family)
    img = psdr.PathTracer(DEPTH).renderD(sc, 1, seed=5)
    wimg, wd = orc.OracleScene(spec, [0, 1, 2]).render_d(sensor=1, max_depth=DEPTH, seeds=(5, 5, 5))
    assert product.rel_l2(img.detach().cpu().numpy(), wimg) < TOL
    w = torch.linspace(0.5, 1.5, img.numel(), device=img.device).reshape(img.shape)
    assert float(psdr.forward_grad(img, leaves["C0"]).abs().max()) == 0.0          # Sensor[0]'s pose does not reach Sensor[1]'s image
    want = _forward_values(psdr, img, w, leaves)
    (img * w).sum().backward()
    got = _grad_values(leaves)
    print(family, "forward", want, "reverse", got)
    for name in ("P", "albedo", "C1"):
        assert leaves[name].grad is not None and abs(want[name]) > 1e-3 and abs(got[name] - want[name]) < _bound(name, want[name]), (name, got[name], want[name])
    assert want["C0"] == 0.0 and got["C0"] == 0.0
    ref_P = float((wd.astype(np.float64) * w.cpu().numpy().astype(np.float64)).sum())
    assert abs(got["P"] - ref_P) < _bound("P", ref_P), (got["P"], ref_P)


def test_reverse_mode_two_views_in_one_graph(psdr, orc):
    import torch
    sc, leaves, spec = _leafy_scene(psdr, "cbox")
    integ = psdr.PathTracer(DEPTH)
    img0, img1 = integ.renderD(sc, 0, seed=5), integ.renderD(sc, 1, seed=6)
    w = torch.linspace(0.5, 1.5, img0.numel(), device=img0.device).reshape(img0.shape)
    ref = orc.OracleScene(spec, [0, 1, 2])
    for k, img, seed in ((0, img0, 5), (1, img1, 6)):
        assert product.rel_l2(img.detach().cpu().numpy(), ref.render_d(sensor=k, max_depth=DEPTH, seeds=(seed, seed, seed))[0]) < TOL
    view0, view1 = _forward_values(psdr, img0, w, leaves), _forward_values(psdr, img1, w, leaves)
    print("view 0", view0, "view 1", view1)
    assert view0["C1"] == 0.0 and view1["C0"] == 0.0                               # each pose reaches its own view only
    ((img0 * w).sum() + (img1 * w).sum()).backward(retain_graph=True)             # (both pairs hang on the same leaf -> matrix expressions)
    first = _grad_values(leaves)
    for name in leaves:
        want = view0[name] + view1[name]
        assert abs(view0[name]) + abs(view1[name]) > 1e-3 and abs(first[name] - want) < _bound(name, want), (name, first[name], view0[name], view1[name])
    # a fresh pair, rendered in the other order: the same gradients (the same samples; only the order of the float sums differs)
    for t in leaves.values():
        t.grad = None
    img1, img0 = integ.renderD(sc, 1, seed=6), integ.renderD(sc, 0, seed=5)
    ((img0 * w).sum() + (img1 * w).sum()).backward()
    second = _grad_values(leaves)
    print("first", first, "second", second)
    for name in leaves:
        assert abs(second[name] - first[name]) <= 1e-5 * max(1.0, abs(first[name])), (name, first[name], second[name])


# --------------------------------------------------------------------------------------------------------------------------- k. incremental update of one sensor
def test_moving_one_sensor_leaves_the_other_alone(psdr, orc):
    spec = cases.family_spec("cbox")
    sc = product.build_scene(spec, active=(0, 1))
    integ = psdr.PathTracer(DEPTH)
    mask0 = _live_mask(sc, 0)[0]
    img0 = integ.renderC(sc, 0, seed=3).cpu().numpy()
    mask1_before = _live_mask(sc, 1)[0]
    c = (scenes.translate(150.0, 400.0, -620.0) @ scenes._rot_x(np.radians(18.0))).astype(np.float32)
    dC = np.zeros((4, 4), np.float32); dC[0, 3] = 50.0
    sc.param_map["Sensor[1]"]._set("to_world", c, dC)
    spec.cameras[1].to_world_raw, spec.cameras[1].d_to_world_raw = c, dC
    sc.configure([0, 1])
    assert sc._last_update()["tree"] == "kept"
    fresh, ref = product.build_scene(spec, active=(0, 1)), orc.OracleScene(spec, [0, 1])
    # sensor 1: image, derivative and mask of the new pose
    _check_terms(psdr, orc, sc, ref, 1, "moved sensor")
    for terms in (orc.TERM_INTERIOR, orc.TERM_PRIMARY, orc.TERM_SECONDARY):
        got, want = psdr.render_d_fwd(integ, sc, 1, seed=5, terms=terms), psdr.render_d_fwd(integ, fresh, 1, seed=5, terms=terms)
        assert float(want[1].abs().max()) > 0 and product.rel_l2(got[1].cpu().numpy(), want[1].cpu().numpy()) < FRESH_TOL, terms
        if terms & orc.TERM_INTERIOR:
            assert product.rel_l2(got[0].cpu().numpy(), want[0].cpu().numpy()) < FRESH_TOL
    mask1 = _check_live_mask(sc, 1, "moved sensor")
    assert np.array_equal(mask1, _live_mask(fresh, 1)[0]) and not np.array_equal(mask1, mask1_before)
    # sensor 0 did not move: the same mask words, the same image bit for bit, the oracle's derivative
    assert np.array_equal(_live_mask(sc, 0)[0], mask0)
    assert np.array_equal(integ.renderC(sc, 0, seed=3).cpu().numpy(), img0)
    _check_terms(psdr, orc, sc, ref, 0, "sensor that stayed")


def test_rendering_both_sensors_from_device_selected_edges(psdr, orc, monkeypatch):
    """tests/test_gpu_device_edges.py compares the edge arrays the device selects with the host's; this renders through them: with the gate lifted, after two vertex
    moves the primary edges of both sensors are the device's own selection, and each sensor's terms are the oracle's for that sensor"""
    from test_gpu_device_edges import _spec
    monkeypatch.setenv("PSDR_DEVICE_EDGES_MIN", "0")
    spec = _spec()
    sc = product.build_scene(spec, active=(0, 1))
    mesh = sc.param_map["Mesh[0]"]
    v0 = np.asarray(spec.meshes[0].vertices, np.float32)
    for scale in (0.99, 0.97):      # the first update after the create sizes the edge arrays, from the second on the device selects
        v = v0.copy(); v[:, 1] *= scale
        dv = np.zeros_like(v); dv[:, 2] = 0.5 * v[:, 0]
        mesh._set("vertex_positions", v, dv)
        sc.configure([0, 1])
    spec.meshes[0].vertices, spec.meshes[0].d_vertices, spec.meshes[0].path = v, dv, None
    assert sc._last_update()["edge_path"] == "device" and sc._check_device_edges() == 0
    ref = orc.OracleScene(spec, [0, 1])
    assert ref.num_primary_edges(0) != ref.num_primary_edges(1)
    for k in (0, 1):
        assert np.abs(ref.render_d(sensor=k, max_depth=DEPTH, seeds=(5, 5, 5), terms=orc.TERM_PRIMARY)[1]).max() > 0
        _check_terms(psdr, orc, sc, ref, k, "device edges")
