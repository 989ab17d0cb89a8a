"""GPU tests of the differentiable Scene.unit_ray_intersectAD (reference psdr.cpp:405, scene.cpp:774-797 with ad = true, path_space = false):
the record's members carry derivatives with respect to the rays' o / d and the meshes' vertex positions and transforms, in reverse mode
(psdr_hip_ray_intersect_adj + the host chain rule) and in forward mode (psdr_hip_ray_intersect_ad with tangents)."""

import numpy as np
import pytest

import product
import scenes

pytestmark = pytest.mark.gpu

FLOOR = 3                       # the floor's mesh index in scenes.cbox_scene / sphere_scene


@pytest.fixture(scope="module")
def psdr():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists)")
    import __graft_entry__
    __graft_entry__.build()
    import psdr_jit_amd
    return psdr_jit_amd


def _members(its):
    return [its.t, its.p, its.n, its.sh_frame.s, its.sh_frame.t, its.sh_frame.n, its.wi, its.uv]


def _rel_l2(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _floor_transform(psdr, sc, P):
    """the floor moved by P along its normal (+y)"""
    sc.param_map["Mesh[%d]" % FLOOR].set_transform(psdr.Matrix4fD([[1., 0., 0., 0.], [0., 1., 0., P], [0., 0., 1., 0.], [0., 0., 0., 1.]]))
    sc.configure([0])


def _open_floor_rays(n, seed, y=200.0, tilt=0.03):
    """rays pointed down at the open floor beside the two boxes (x in [25, 60] or [495, 535]): nothing in the way for floor heights 0..20"""
    rng = np.random.default_rng(seed)
    x = np.where(rng.random(n) < 0.5, rng.uniform(25.0, 60.0, n), rng.uniform(495.0, 535.0, n))
    o = np.stack([x, np.full(n, y), rng.uniform(30.0, 530.0, n)], axis=1).astype(np.float32)
    d = np.stack([rng.uniform(-tilt, tilt, n), -np.ones(n), rng.uniform(-tilt, tilt, n)], axis=1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o, d.astype(np.float32)


def _random_rays(n, seed):
    rng = np.random.default_rng(seed)
    o = np.tile(np.array([[278.0, 273.0, -300.0]], np.float32), (n, 1)) + rng.normal(0, 20, (n, 3)).astype(np.float32)
    d = rng.normal(0, 1, (n, 3)).astype(np.float32)
    d[:, 2] = np.abs(d[:, 2]) + 0.3
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o, d


# ---------------------------------------------------------------------------------------------------- the float64 restatement
def restate(o, d, rows, uv, flat):
    """Scene::ray_intersect<true, false> (scene.cpp:774-797) for rays o, d [m, 3] on their hit triangles' rows [m, 22] ([p0 e1 e2 n0 n1 n2
    face_normal area]), corner texture coordinates uv [m, 6] and flat-shading flags [m], in torch float64 -> the members in IntersectionD's
    order (t, p, n, sh_frame.s, .t, .n, wi, uv)"""
    import torch
    p0, e1, e2, n0, n1, n2, fn = (rows[:, 3 * k:3 * k + 3] for k in range(7))
    dot = lambda a, b: (a * b).sum(1)
    h = torch.cross(d, e2, dim=1)
    f = 1.0 / dot(e1, h)
    s = o - p0
    q = torch.cross(s, e1, dim=1)
    u, v, t = f * dot(s, h), f * dot(d, q), f * dot(e2, q)
    p = o + t[:, None] * d
    nb = n0 + (n1 - n0) * u[:, None] + (n2 - n0) * v[:, None]
    nb_len = torch.where(flat, torch.ones_like(u), nb.norm(dim=1))
    sh = torch.where(flat[:, None], fn, nb / nb_len[:, None])
    uv0, du0, du1 = uv[:, 0:2], uv[:, 2:4] - uv[:, 0:2], uv[:, 4:6] - uv[:, 0:2]
    det = du0[:, 0] * du1[:, 1] - du0[:, 1] * du1[:, 0]
    has_uv = det != 0
    inv_det = 1.0 / torch.where(has_uv, det, torch.ones_like(det))
    dp_du = (e1 * du1[:, 1:2] - e2 * du0[:, 1:2]) * inv_det[:, None]
    dp_du = torch.where(has_uv[:, None], dp_du, torch.tensor([1.0, 0.0, 0.0], dtype=dp_du.dtype).expand_as(dp_du))
    w = dp_du - sh * dot(sh, dp_du)[:, None]
    w_len = torch.where(has_uv, w.norm(dim=1), torch.ones_like(u))
    fs_uv = w / w_len[:, None]
    ft_uv = torch.cross(sh, fs_uv, dim=1)
    sg = torch.where(sh[:, 2].detach() < 0, -1.0, 1.0).to(sh.dtype)          # Duff et al. (frame.h:9-28)
    a = -1.0 / (sg + sh[:, 2])
    b = sh[:, 0] * sh[:, 1] * a
    fs_d = torch.stack([sg * sh[:, 0] ** 2 * a + 1.0, sg * b, -sg * sh[:, 0]], dim=1)
    ft_d = torch.stack([b, sg + sh[:, 1] ** 2 * a, -sh[:, 1]], dim=1)
    fs = torch.where(has_uv[:, None], fs_uv, fs_d)
    ft = torch.where(has_uv[:, None], ft_uv, ft_d)
    wi = torch.stack([dot(-d, fs), dot(-d, ft), dot(-d, sh)], dim=1)
    tex = uv0 + du0 * u[:, None] + du1 * v[:, None]
    return [t, p, fn, fs, ft, sh, wi, tex]


def _snapshot_rows(sc, leaf64):
    """float64 rows of every triangle: differentiable (chain.snapshot_tensors over the given leaves) for the meshes with a leaf, the
    configured rows as constants for the others; with the corner uvs and flat flags"""
    import torch
    from psdr_jit_amd import chain
    snap = sc._snapshot()
    tri32 = torch.as_tensor(np.asarray(snap["triangles"], np.float64))
    tri64 = chain.snapshot_tensors(sc, 0, lambda obj, name: leaf64.get((id(obj), name), chain._t(obj._get(name, False))))[0]
    mesh_id = np.asarray(snap["mesh_id"])
    moved = np.zeros(len(mesh_id), bool)
    for (oid, _name) in leaf64:
        for i in range(sc.num_meshes):
            if id(sc.param_map.get("Mesh[%d]" % i)) == oid:
                moved |= mesh_id == i
    rows = torch.where(torch.as_tensor(moved)[:, None], tri64, tri32)
    flat = np.array([bool(sc.param_map["Mesh[%d]" % m].use_face_normal) for m in mesh_id])
    return rows, torch.as_tensor(np.asarray(snap["uv"], np.float64).reshape(-1, 6)), torch.as_tensor(flat), mesh_id


# ---------------------------------------------------------------------------------------------------- 1. closed form
def test_floor_translation_closed_form(psdr):
    """rays hitting the floor, whose transform carries P along its normal: dt/dP = 1/d_y, dp/dP = d/d_y exactly"""
    import torch
    sc = product.build_scene(scenes.cbox_scene(16, 16, 1, 0, 0, param=None))
    P = psdr.FloatD(0.).requires_grad_()
    _floor_transform(psdr, sc, P)
    o, d = _open_floor_rays(4096, 1)
    gen = torch.Generator().manual_seed(1)
    w_t, w_p = torch.rand(4096, generator=gen) + 0.5, torch.rand(4096, 3, generator=gen) - 0.5
    its = sc.unit_ray_intersectAD(psdr.RayC(torch.from_numpy(o), torch.from_numpy(d)))
    assert bool(its.is_valid().all()) and bool((its.shape == FLOOR).all())
    dy = d[:, 1].astype(np.float64)
    want_t = float((w_t.double().numpy() / dy).sum())
    want_p = float(((w_p.double().numpy() * d) / dy[:, None]).sum())
    (its.t * w_t.to(its.t.device)).sum().backward(retain_graph=True)
    assert abs(float(P.grad) - want_t) < 1e-4 * abs(want_t), (float(P.grad), want_t)
    P.grad = None
    (its.p * w_p.to(its.p.device)).sum().backward()
    assert abs(float(P.grad) - want_p) < 1e-4 * abs(want_p), (float(P.grad), want_p)
    its = sc.unit_ray_intersectAD(psdr.RayC(torch.from_numpy(o), torch.from_numpy(d)))
    dt = psdr.forward_grad(its.t, P).cpu().numpy().astype(np.float64)
    assert np.allclose(dt, 1.0 / dy, rtol=1e-5)
    fwd_t = float((w_t.double().numpy() * dt).sum())
    assert abs(fwd_t - want_t) < 1e-4 * abs(want_t)
    dp = psdr.forward_grad(its.p, P).cpu().numpy().astype(np.float64)
    assert np.allclose(dp, d / dy[:, None], rtol=1e-5, atol=1e-6)


# ---------------------------------------------------------------------------------------------------- 2. reverse mode vs float64
def _cbox_with_translation(psdr, torch):
    sc = product.build_scene(scenes.cbox_scene(16, 16, 1, 0, 0, param=None))
    m = sc.param_map["Mesh[1]"]                                     # the small box: a 4 x 4 leaf (translation 0)
    L = torch.eye(4, dtype=torch.float32).requires_grad_()
    m.to_world_left = L
    sc.configure([0])
    return sc, [(m, "to_world_left", L)], scenes.cbox_scene(16, 16, 1, 0, 0, param=None)


def _sphere_with_vertices(psdr, torch):
    spec = scenes.sphere_scene(16, 16, 1, 0, 0)
    sc = product.build_scene(spec)
    m = sc.param_map["Mesh[2]"]                                     # the large ball: 304 triangles, smooth vertex normals (BVH class)
    V = torch.tensor(np.asarray(m._get("vertex_positions", False)), dtype=torch.float32).reshape(-1, 3).requires_grad_()
    m.vertex_positions = V
    sc.configure([0])
    return sc, [(m, "vertex_positions", V)], spec


def _textured_with_vertices(psdr, torch):
    spec = scenes.textured_scene(16, 16, 1, 0, 0, env=False)
    sc = product.build_scene(spec)
    m = sc.param_map["Mesh[0]"]                                     # the uv-mapped floor: the uv output and the dp_du frame
    V = torch.tensor(np.asarray(m._get("vertex_positions", False)), dtype=torch.float32).reshape(-1, 3).requires_grad_()
    m.vertex_positions = V
    sc.configure([0])
    return sc, [(m, "vertex_positions", V)], spec


@pytest.mark.parametrize("make", [_cbox_with_translation, _sphere_with_vertices, _textured_with_vertices], ids=["cbox_translation", "sphere_vertices", "textured_floor"])
def test_reverse_mode_matches_float64_restatement(psdr, orc, make):
    import torch
    sc, leaves, spec = make(psdr, torch)
    n = 4096
    o_np, d_np = _random_rays(n, 7)
    if make is _textured_with_vertices:
        d_np[:, 1] = -np.abs(d_np[:, 1]) - 0.2                        # most rays down at the floor
        d_np /= np.linalg.norm(d_np, axis=1, keepdims=True)
    o, d = torch.from_numpy(o_np).requires_grad_(), torch.from_numpy(d_np).requires_grad_()
    its = sc.unit_ray_intersectAD(psdr.RayC(o, d))
    ref = orc.OracleScene(spec, [0])
    tri, _uv, _t = ref.trace(o_np, d_np)
    valid = its.is_valid().cpu().numpy()
    assert np.array_equal(valid, tri >= 0) and valid.sum() > 500
    # weights: random on every float member, zero on misses and on grazing rays (float32 Moller-Trumbore is ill-conditioned there)
    cos = np.abs((its.n.detach().cpu().numpy() * d_np).sum(1))
    keep = valid & (cos >= 0.05)
    print("%s: %d of %d valid rays dropped as grazing (|cos| < 0.05)" % (make.__name__, int((valid & ~keep).sum()), int(valid.sum())))
    assert keep.sum() > 0.8 * valid.sum()
    gen = torch.Generator().manual_seed(3)
    members = _members(its)
    W = [(torch.rand(tuple(m.shape), generator=gen, dtype=torch.float64) - 0.5) * torch.as_tensor(keep).reshape((-1,) + (1,) * (m.dim() - 1)) for m in members]
    loss = sum((m * w.to(m.device, torch.float32)).sum() for m, w in zip(members, W))
    loss.backward()
    for m in members:
        assert m.grad_fn is members[0].grad_fn
    # reference: torch autograd of the solid-angle formulas on the oracle's hit triangles, float64
    leaf64 = {(id(obj), name): t.detach().to(torch.float64).clone().requires_grad_() for obj, name, t in leaves}
    rows, uvs, flat, _mesh = _snapshot_rows(sc, leaf64)
    idx = np.nonzero(keep)[0]
    k = torch.as_tensor(tri[idx].astype(np.int64))
    o64, d64 = o.detach().double().requires_grad_(), d.detach().double().requires_grad_()
    ms = restate(o64[idx], d64[idx], rows[k], uvs[k], flat[k])
    ref_loss = sum((m_ * w[idx].reshape(m_.shape)).sum() for m_, w in zip(ms, W))
    ref_loss.backward()
    for (obj, name, t) in leaves:
        g, want = t.grad.numpy(), leaf64[(id(obj), name)].grad.numpy()
        assert np.isfinite(g).all()
        e = _rel_l2(g, want)
        assert e <= 1e-4, (name, e)
    for got, want in ((o.grad, o64.grad), (d.grad, d64.grad)):
        assert got.device.type == "cpu" and got.dtype == torch.float32 and np.isfinite(got.numpy()).all()
        e = _rel_l2(got.numpy(), want.numpy())
        assert e <= 1e-4, e
    # the primal values of the restatement are the record's
    for m, m64 in zip(members, ms):
        assert _rel_l2(m.detach().cpu().numpy()[idx], m64.detach().numpy()) < 1e-5


# ---------------------------------------------------------------------------------------------------- 3. forward vs reverse on the device
def _clear_spec_tangents(sc):
    """scenes.sphere_scene gives the luminaire and the small ball a forward tangent through the host objects (d_to_world_left): forward mode
    carries tangents set that way along with the parameter's own (as renderD's does) - zero them, so that forward_grad sees d / dP alone"""
    for i in range(sc.num_meshes):
        m = sc.param_map["Mesh[%d]" % i]
        for name in ("to_world_left", "to_world", "to_world_right"):
            v = np.asarray(m._get(name, False), np.float32).reshape(4, 4)
            m._set(name, v, np.zeros_like(v))


def test_forward_mode_matches_reverse_mode(psdr):
    """sum_i <w_i, forward_grad(member_i, P, v)> = <backward() gradient of P, v>, P moving the ball's vertices and the rays"""
    import torch
    sc = product.build_scene(scenes.sphere_scene(16, 16, 1, 0, 0))
    _clear_spec_tangents(sc)
    m = sc.param_map["Mesh[2]"]
    V0 = torch.tensor(np.asarray(m._get("vertex_positions", False)), dtype=torch.float32).reshape(-1, 3)
    P = torch.zeros(3, requires_grad=True)
    m.vertex_positions = V0 + P
    sc.configure([0])
    o_np, d_np = _random_rays(4096, 11)
    o = torch.from_numpy(o_np) + 0.5 * P
    d = torch.from_numpy(d_np) + 0.01 * P
    its = sc.unit_ray_intersectAD(psdr.RayC(o, d))
    members = _members(its)
    valid = its.is_valid().cpu().numpy()
    cos = np.abs((its.n.detach().cpu().numpy() * d_np).sum(1))
    keep = torch.as_tensor(valid & (cos >= 0.05))
    gen = torch.Generator().manual_seed(5)
    W = [((torch.rand(tuple(x.shape), generator=gen) - 0.5) * keep.reshape((-1,) + (1,) * (x.dim() - 1))).to(x.device) for x in members]
    v = torch.tensor([0.3, -1.0, 0.7])
    fwd = sum(float((psdr.forward_grad(x, P, v).double() * w.double()).sum()) for x, w in zip(members, W))
    sum((x * w).sum() for x, w in zip(members, W)).backward()
    rev = float((P.grad.double() * v.double()).sum())
    assert abs(fwd - rev) <= 1e-4 * max(abs(rev), abs(fwd)), (fwd, rev)
    assert abs(rev) > 1e-2


# ---------------------------------------------------------------------------------------------------- 4. primal and edges
@pytest.mark.parametrize("which", ["cbox", "sphere", "textured"])
def test_primal_record_equals_the_c_record(psdr, which):
    import torch
    spec = {"cbox": lambda: scenes.cbox_scene(16, 16, 1, 0, 0, param=None), "sphere": lambda: scenes.sphere_scene(16, 16, 1, 0, 0),
            "textured": lambda: scenes.textured_scene(16, 16, 1, 0, 0, env=False)}[which]()
    sc = product.build_scene(spec)
    o, d = _random_rays(4096, 2)
    ray = psdr.RayC(torch.from_numpy(o), torch.from_numpy(d))
    c = sc.unit_ray_intersect(ray)
    a = sc.unit_ray_intersectAD(ray)
    assert isinstance(a, psdr.IntersectionD)
    valid = c.is_valid()
    assert torch.equal(valid, a.is_valid()) and torch.equal(c.shape, a.shape) and torch.equal(c.J, a.J)
    assert int(valid.sum()) > 200
    vm = valid.cpu().numpy()
    for x, y in zip(_members(c), _members(a)):
        assert not y.requires_grad
        assert _rel_l2(y.cpu().numpy()[vm], x.cpu().numpy()[vm]) < 1e-5


def test_misses_inactive_rays_and_reconfigure(psdr):
    import torch
    sc = product.build_scene(scenes.cbox_scene(16, 16, 1, 0, 0, param=None))
    m = sc.param_map["Mesh[1]"]
    L = torch.eye(4, dtype=torch.float32).requires_grad_()
    m.to_world_left = L
    sc.configure([0])
    n = 2048
    o_np, d_np = _random_rays(n, 9)
    d_np[: n // 4, 2] = -np.abs(d_np[: n // 4, 2])                # out through the open front: misses
    rng = np.random.default_rng(9)
    active = rng.random(n) < 0.7
    o, d = torch.from_numpy(o_np).requires_grad_(), torch.from_numpy(d_np).requires_grad_()
    its = sc.unit_ray_intersectAD(psdr.RayC(o, d), active=torch.from_numpy(active))
    hit = (its.shape >= 0).cpu().numpy()
    assert (~hit).sum() > n // 8 and (hit & ~active).sum() > 100
    assert np.array_equal(its.is_valid().cpu().numpy(), hit & active)
    sum(x.sum() for x in _members(its)).backward()
    off = ~(hit & active)
    assert np.all(o.grad.numpy()[off] == 0.0) and np.all(d.grad.numpy()[off] == 0.0)
    assert np.abs(o.grad.numpy()[~off]).sum() > 0
    for g in (o.grad, d.grad, L.grad):
        assert np.isfinite(g.numpy()).all()
    # nothing requires grad: nothing is attached
    its2 = sc.unit_ray_intersectAD(psdr.RayC(torch.from_numpy(o_np), torch.from_numpy(d_np)))
    m.to_world_left = torch.eye(4, dtype=torch.float32)
    sc.configure([0])
    its3 = sc.unit_ray_intersectAD(psdr.RayC(torch.from_numpy(o_np), torch.from_numpy(d_np)))
    assert not any(x.requires_grad for x in _members(its3))
    # a configure() between the call and backward(): an error, not gradients through other rows
    with pytest.raises(RuntimeError, match="configured again"):
        sum(x.sum() for x in _members(its2)).backward()
    # the C ABI: misses, a slot outside the scene and all-zero adjoints add nothing to any row
    from psdr_jit_amd import cabi
    L_ = cabi.lib()
    n_tris = int(sc._snapshot_counts()[0])
    dev = torch.device("cuda")
    oo, dd = torch.from_numpy(o_np).to(dev), torch.from_numpy(d_np).to(dev)
    hits = torch.full((n,), -1, dtype=torch.int32, device=dev)
    hits[::3] = n_tris + 5
    hits[1::3] = 2**30
    g_rec = torch.ones((n, 24), dtype=torch.float32, device=dev)
    g_tri = torch.zeros(n_tris * 22, dtype=torch.float32, device=dev)
    g_o = torch.full((n, 3), 7.0, device=dev)
    g_d = torch.full((n, 3), 7.0, device=dev)
    cabi.check(L_.psdr_hip_ray_intersect_adj(sc._hip_handle(), n, oo.data_ptr(), dd.data_ptr(), hits.data_ptr(), g_rec.data_ptr(), None,
                                             g_tri.data_ptr(), g_o.data_ptr(), g_d.data_ptr(), None))
    torch.cuda.synchronize()
    assert float(g_tri.abs().sum()) == 0.0 and float(g_o.abs().sum()) == 0.0 and float(g_d.abs().sum()) == 0.0
    assert L_.psdr_hip_ray_intersect_adj(None, n, oo.data_ptr(), dd.data_ptr(), hits.data_ptr(), g_rec.data_ptr(), None, None, None, None, None) != 0
    assert L_.psdr_hip_ray_intersect_ad(sc._hip_handle(), n, None, dd.data_ptr(), None, None, g_rec.data_ptr(), None, hits.data_ptr(), None) != 0


# ---------------------------------------------------------------------------------------------------- 5. contention and reproducibility
def _camera_rays(res):
    """rays of the README camera (fov 60, at (208, 273, -800) looking down +z) through a res x res grid of pixel centres"""
    tan = np.tan(np.radians(30.0))
    ys, xs = np.meshgrid((np.arange(res) + 0.5) / res, (np.arange(res) + 0.5) / res, indexing="ij")
    d = np.stack([(1.0 - 2.0 * xs) * tan, (1.0 - 2.0 * ys) * tan, np.ones_like(xs)], axis=-1).reshape(-1, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = np.tile(np.array([[208.0, 273.0, -800.0]]), (d.shape[0], 1))
    return o.astype(np.float32), d.astype(np.float32)


@pytest.mark.parametrize("rounds", [None, "0"])
def test_contended_floor_rows_and_reproducibility(psdr, orc, monkeypatch, rounds):
    """1 M camera rays of the Cornell box: every floor hit adds to one of two rows.  The floor rows of g_triangles match a float64 sum of the
    per-ray restatement, and ten launches agree to 1e-5 of the buffer's L1 norm (the rule for float atomics).  rounds = "0": per-lane atomics."""
    import torch
    from psdr_jit_amd import cabi
    if rounds is not None:
        monkeypatch.setenv("PSDR_ISECT_ADJ_ROUNDS", rounds)
    spec = scenes.cbox_scene(16, 16, 1, 0, 0, param=None)
    sc = product.build_scene(spec)
    L_ = cabi.lib()
    o_np, d_np = _camera_rays(1024)
    n = o_np.shape[0]
    dev = torch.device("cuda")
    o, d = torch.from_numpy(o_np).to(dev), torch.from_numpy(d_np).to(dev)
    rec = torch.zeros((n, 24), dtype=torch.float32, device=dev)
    hit = torch.empty((n,), dtype=torch.int32, device=dev)
    cabi.check(L_.psdr_hip_ray_intersect_ad(sc._hip_handle(), n, o.data_ptr(), d.data_ptr(), None, None, rec.data_ptr(), None, hit.data_ptr(), None))
    torch.cuda.synchronize()
    gen = torch.Generator().manual_seed(8)
    g_rec = (torch.rand((n, 24), generator=gen) - 0.5)
    g_rec[:, [0, 1, 3]] = 0.0
    valid = (rec[:, 0] > 0).cpu()
    g_rec[~valid] = 0.0
    g_rec_d = g_rec.to(dev)
    n_tris = int(sc._snapshot_counts()[0])
    runs = []
    for _ in range(10):
        g_tri = torch.zeros(n_tris * 22, dtype=torch.float32, device=dev)
        cabi.check(L_.psdr_hip_ray_intersect_adj(sc._hip_handle(), n, o.data_ptr(), d.data_ptr(), hit.data_ptr(), g_rec_d.data_ptr(), None,
                                                 g_tri.data_ptr(), None, None, None))
        torch.cuda.synchronize()
        runs.append(g_tri.cpu().numpy().astype(np.float64).reshape(n_tris, 22))
    l1 = np.abs(runs[0]).sum()
    for r in runs[1:]:
        assert np.abs(r - runs[0]).sum() <= 1e-5 * l1
    assert np.all(runs[0][:, 21] == 0.0)                               # face_area: J = 1
    # float64: per-ray row adjoints of the floor hits (on the triangles the oracle's trace reports), summed
    rows, uvs, flat, mesh_id = _snapshot_rows(sc, {})
    snap_floor = np.nonzero(mesh_id == FLOOR)[0]
    rec_np = rec.cpu().numpy()
    on_floor = valid.numpy() & (rec_np[:, 1] == FLOOR)
    assert on_floor.sum() > 30000                                      # on two triangles
    tri, _uv, _t = orc.OracleScene(spec, [0]).trace(o_np[on_floor], d_np[on_floor])
    assert np.all(mesh_id[tri] == FLOOR)
    best = torch.as_tensor(tri.astype(np.int64))
    o64 = torch.as_tensor(o_np[on_floor].astype(np.float64))
    d64 = torch.as_tensor(d_np[on_floor].astype(np.float64))
    R = rows[best].clone().requires_grad_()
    ms = restate(o64, d64, R, uvs[best], flat[best])
    g = g_rec[on_floor].double()
    loss = sum((m_ * g[:, a:a + w].reshape(m_.shape)).sum() for m_, (a, w) in zip(ms, ((2, 1), (4, 3), (7, 3), (10, 3), (13, 3), (16, 3), (19, 3), (22, 2))))
    loss.backward()
    want = torch.zeros((n_tris, 22), dtype=torch.float64).index_add_(0, best, R.grad).numpy()
    for k in snap_floor:
        e = _rel_l2(runs[0][k, :21], want[k, :21])
        assert e <= 1e-4, (int(k), e)


# ---------------------------------------------------------------------------------------------------- 6. a short optimisation
def test_depth_optimisation_recovers_the_floor_offset(psdr):
    import torch
    sc = product.build_scene(scenes.cbox_scene(16, 16, 1, 0, 0, param=None))
    o_np, d_np = _open_floor_rays(2048, 4)
    ray = psdr.RayC(torch.from_numpy(o_np), torch.from_numpy(d_np))
    _floor_transform(psdr, sc, 20.0)
    target = sc.unit_ray_intersect(ray)
    assert bool(target.is_valid().all()) and bool((target.shape == FLOOR).all())
    t_star = target.t.clone()
    P = torch.zeros((), requires_grad=True)
    for _ in range(30):
        _floor_transform(psdr, sc, P)
        its = sc.unit_ray_intersectAD(ray)
        loss = ((its.t - t_star) ** 2).mean()
        P.grad = None
        loss.backward()
        with torch.no_grad():
            P -= 0.25 * P.grad
    assert abs(float(P.detach()) - 20.0) < 1e-2, float(P.detach())
