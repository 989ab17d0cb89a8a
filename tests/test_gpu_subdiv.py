"""GPU tests of mesh subdivision as an operator (psdr_jit_amd/subdiv.py, csrc/hip/subdiv.hip): refine = S x and restrict = S^T y against the float64
matrix of tests/subdiv_ref.py, the inner-product identity between the two, the tetrahedron's known answer bit for bit, repeatability, both autograd
functions, chained levels, the uv operator, the gradient of a rendered image arriving at a control cage, and every refusal.

The bound is derived, not tuned.  An output row with k entries is k fused multiply-adds from 0 over float32 weights, each within 2 ulp of its float64
value (one rounding of the weight, and of beta and 1 - d beta had they been formed in float32):
    |y_r - (S64 x)_r| <= gamma_{k + 4} sum_j |S64_rj| |x_j|,     gamma_m = m u / (1 - m u),  u = 2^-24
A chain of levels is compared level by level, each level fed the device's own previous output.

The meshes: the tetrahedron, `bowtie`, `book`, the 200-fan (hub row: 201 entries forward and, its rim being a boundary, 201 transposed), a
200-gon bipyramid (closed, so a hub's transpose row has 601 entries: the long row one lane walks alone), the bunny at two levels and a 257 x 257 grid,
whose fine level has 263 169 rows - more than one pass of the 1024 x 256 launch grid, so the grid-stride loop runs."""
import os

import numpy as np
import pytest

import scenes
import subdiv_ref as ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
BALL = os.path.join(scenes.DATA, "cbox_smallball.obj")
LARGEBOX = os.path.join(scenes.DATA, "cbox_largebox.obj")
MESHES = ["tetrahedron", "bowtie", "book", "fan", "bipyramid", "bunny", "grid"]
TETRA_ROWS = [(3, 3, 3), (7, 3, 3), (3, 7, 3), (3, 3, 7), (6, 2, 2), (2, 6, 2), (2, 2, 6), (6, 6, 2), (6, 2, 6), (2, 6, 6)]


@pytest.fixture(scope="module")
def psdr():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists)")
    import __graft_entry__
    __graft_entry__.build()
    import psdr_jit_amd
    return psdr_jit_amd


def _bipyramid(k):
    """hubs 0 and 1 over the rim 2 .. k + 1: closed, every edge interior, both hubs of valence k"""
    faces = []
    for i in range(k):
        a, b = 2 + i, 2 + (i + 1) % k
        faces += [[0, a, b], [1, b, a]]
    return faces, k + 2


_MESH = {}


def _mesh(name):
    """(faces, n, levels)"""
    if name not in _MESH:
        if name == "tetrahedron":
            m = (ref.TETRAHEDRON, 4, 1)
        elif name == "bowtie":
            m = (ref.BOWTIE, 5, 1)
        elif name == "book":
            m = (ref.BOOK, 5, 1)
        elif name == "fan":
            m = ref.fan(200) + (1,)
        elif name == "bipyramid":
            m = _bipyramid(200) + (1,)
        elif name == "bunny":
            m = ref.load_obj(ref.BUNNY)[:2] + (2,)
        else:
            m = ref.grid(257) + (1,)
        _MESH[name] = (np.asarray(m[0], np.int32), m[1], m[2])
    return _MESH[name]


_SUBS = {}


def _setup(psdr, name, scheme):
    """([one single-level Subdivision per level, chained], [S64 per level]) per mesh and scheme, built once and shared"""
    if (name, scheme) not in _SUBS:
        faces, n, levels = _mesh(name)
        chain = ref.reference_chain(name, faces, n, scheme, levels)
        subs, f, m = [], faces, n
        for _ in range(levels):
            subs.append(psdr.Subdivision(f, m, levels=1, scheme=scheme))
            f, m = subs[-1].faces, subs[-1].num_vertices_out
        for s, (S64, fine, E, _sharp) in zip(subs, chain):
            assert s.num_vertices_out == S64.shape[0] and s.num_vertices_in == S64.shape[1] and np.array_equal(s.faces, np.array(fine))
        _SUBS[(name, scheme)] = (subs, [c[0] for c in chain])
    return _SUBS[(name, scheme)]


def _gamma(k):
    m = np.asarray(k, np.float64) + 4.0
    return m * U / (1.0 - m * U)


def _bounds(S64, x, transpose):
    """(want, bound) of S64 x, or of S64^T x, per entry; x float32 values taken to float64"""
    A = S64.T.tocsr() if transpose else S64
    x = np.asarray(x, np.float64)
    k = np.diff(A.indptr)
    return A @ x, _gamma(k)[:, None] * (abs(A) @ np.abs(x))


def _check(got, want, bound, label):
    err = np.abs(np.asarray(got, np.float64) - want)
    print(label, "worst error / bound %.3f" % float((err / np.maximum(bound, 1e-300)).max()), "max |want| %.3f" % float(np.abs(want).max()))
    assert np.isfinite(got).all() and np.all(err <= bound), label


@pytest.mark.parametrize("scheme", ["loop", "linear"])
@pytest.mark.parametrize("name", MESHES)
def test_refine_within_the_bound(psdr, name, scheme):
    import torch
    subs, mats = _setup(psdr, name, scheme)
    if name == "grid":
        assert subs[0].num_vertices_out == 263169 > 1024 * 256
    if name == "bunny":
        assert len(subs) == 2 and subs[1].num_vertices_out == 39826
    rng = np.random.default_rng(26)         # (a seed with which max |want| > 1 on the four- and five-vertex meshes too: the test cannot pass on zeros)
    for C in (1, 2, 3, 4):
        x = torch.from_numpy(rng.standard_normal((subs[0].num_vertices_in, C)).astype(np.float32))
        for l, (sub, S64) in enumerate(zip(subs, mats)):
            y = sub.refine(x)
            assert y.is_cuda and y.dtype == torch.float32 and tuple(y.shape) == (sub.num_vertices_out, C)
            want, bound = _bounds(S64, x.cpu().numpy(), False)
            assert np.abs(want).max() > 1.0
            _check(y.cpu().numpy(), want, bound, "%s %s C=%d level %d" % (name, scheme, C, l))
            x = y


@pytest.mark.parametrize("scheme", ["loop", "linear"])
@pytest.mark.parametrize("name", MESHES)
def test_restrict_within_the_bound(psdr, name, scheme):
    import torch
    subs, mats = _setup(psdr, name, scheme)
    if name == "bipyramid" and scheme == "loop":
        assert np.diff(subs[0].csr(0, transpose=True)[0])[0] == 601
    if name == "fan":
        assert np.diff(subs[0].csr(0, transpose=True)[0])[0] == 201
    rng = np.random.default_rng(8)          # (likewise)
    for C in (1, 2, 3, 4):
        y = torch.from_numpy(rng.standard_normal((subs[-1].num_vertices_out, C)).astype(np.float32))
        for l in reversed(range(len(subs))):
            g = subs[l].restrict(y)
            assert g.is_cuda and g.dtype == torch.float32 and tuple(g.shape) == (subs[l].num_vertices_in, C)
            want, bound = _bounds(mats[l], y.cpu().numpy(), True)
            assert np.abs(want).max() > 1.0
            _check(g.cpu().numpy(), want, bound, "%s %s C=%d level %d transposed" % (name, scheme, C, l))
            y = g


@pytest.mark.parametrize("name", ["fan", "bipyramid", "bunny", "grid"])
def test_inner_products_agree(psdr, name):
    """<S x, y> = <x, S^T y>, both formed in float64 from the device's outputs, within the two bounds' inner products"""
    import torch
    subs, mats = _setup(psdr, name, "loop")
    sub, S64 = subs[0], mats[0]
    rng = np.random.default_rng(13)
    x = rng.standard_normal((sub.num_vertices_in, 3)).astype(np.float32)
    y = rng.standard_normal((sub.num_vertices_out, 3)).astype(np.float32)
    Sx = sub.refine(torch.from_numpy(x)).cpu().numpy().astype(np.float64)
    STy = sub.restrict(torch.from_numpy(y)).cpu().numpy().astype(np.float64)
    lhs, rhs = float((Sx * y).sum()), float((x * STy).sum())
    slack = float((_bounds(S64, x, False)[1] * np.abs(y)).sum() + (_bounds(S64, y, True)[1] * np.abs(x)).sum())
    print(name, "<Sx, y>", lhs, "<x, S^T y>", rhs, "difference", abs(lhs - rhs), "allowed", slack)
    assert abs(lhs) > 1.0 and abs(lhs - rhs) <= slack


def test_tetrahedron_rows_are_bit_equal(psdr):
    import torch
    sub = _setup(psdr, "tetrahedron", "loop")[0][0]
    c = 16.0 * torch.tensor([[0., 0., 0.], [1., 0., 0.], [0., 1., 0.], [0., 0., 1.]])
    assert torch.equal(sub.refine(c).cpu(), torch.tensor(TETRA_ROWS, dtype=torch.float32))


def test_same_input_same_bits(psdr):
    import torch
    sub = _setup(psdr, "grid", "loop")[0][0]
    rng = np.random.default_rng(14)
    x1, x2 = (torch.from_numpy(rng.standard_normal((sub.num_vertices_in, 3)).astype(np.float32)).cuda() for _ in range(2))
    y1, y2 = (torch.from_numpy(rng.standard_normal((sub.num_vertices_out, 3)).astype(np.float32)).cuda() for _ in range(2))
    a, b, c = sub.refine(x1), sub.refine(x2), sub.refine(x1)
    assert torch.equal(a, c) and not torch.equal(a, b)
    a, b, c = sub.restrict(y1), sub.restrict(y2), sub.restrict(y1)
    assert torch.equal(a, c) and not torch.equal(a, b)


def test_autograd_of_both_directions(psdr):
    import torch
    faces, n, _levels = _mesh("bunny")
    sub = psdr.Subdivision(faces, n, levels=2)
    rng = np.random.default_rng(15)
    w = torch.from_numpy(rng.standard_normal((sub.num_vertices_out, 3)).astype(np.float32)).cuda()
    c = torch.from_numpy(rng.standard_normal((n, 3)).astype(np.float32)).cuda().requires_grad_()
    (w * sub.refine(c)).sum().backward()
    assert torch.equal(c.grad, sub.restrict(w))
    w = torch.from_numpy(rng.standard_normal((n, 3)).astype(np.float32)).cuda()
    y = torch.from_numpy(rng.standard_normal((sub.num_vertices_out, 3)).astype(np.float32)).cuda().requires_grad_()
    (w * sub.restrict(y)).sum().backward()
    assert torch.equal(y.grad, sub.refine(w))
    # a CPU float64 leaf gets a CPU float64 gradient
    c64 = torch.from_numpy(rng.standard_normal((n, 2))).requires_grad_()
    out = sub.refine(c64)
    assert out.is_cuda and out.dtype == torch.float32
    out.square().sum().backward()
    assert c64.grad.device.type == "cpu" and c64.grad.dtype == torch.float64 and tuple(c64.grad.shape) == (n, 2)
    assert torch.equal(c64.grad, sub.restrict(2.0 * out.detach()).cpu().double())


def test_levels_chain_and_uv(psdr):
    import torch
    faces, n, _levels = _mesh("bunny")
    for scheme in ("loop", "linear"):
        subs, _mats = _setup(psdr, "bunny", scheme)
        both = psdr.Subdivision(faces, n, levels=2, scheme=scheme)
        assert (both.levels, both.scheme, both.num_vertices_in, both.num_vertices_out) == (2, scheme, n, subs[1].num_vertices_out)
        assert np.array_equal(both.faces, subs[1].faces) and both.faces.dtype == np.int32 and both.face_uv is None and both.num_uv_out is None
        rng = np.random.default_rng(16)
        x = torch.from_numpy(rng.standard_normal((n, 3)).astype(np.float32))
        y = torch.from_numpy(rng.standard_normal((both.num_vertices_out, 3)).astype(np.float32))
        assert torch.equal(both.refine(x), subs[1].refine(subs[0].refine(x)))
        assert torch.equal(both.restrict(y), subs[0].restrict(subs[1].restrict(y)))
        for l in range(2):
            for t in (False, True):
                assert all(np.array_equal(p, q) for p, q in zip(both.csr(l, transpose=t), subs[l].csr(0, transpose=t)))
    # a mesh with a uv set: the uv operator is the midpoint rule over the uv index topology, whatever the scheme
    box = psdr.Mesh()
    box.load(LARGEBOX)
    sub = psdr.Subdivision(box, levels=2, scheme="loop")
    f, m, _v, fuv, uv = ref.load_obj(LARGEBOX)
    assert (sub.num_vertices_in, sub.num_uv_in) == (m, len(uv)) == (8, 21)
    chain = ref.reference_chain("largebox-uv", fuv, len(uv), "linear", 2)
    assert np.array_equal(sub.face_uv, np.array(chain[1][1])) and sub.num_uv_out == chain[1][0].shape[0]
    uv0 = np.asarray(box.vertex_uv, np.float32).reshape(-1, 2)
    got = sub.refine_uv(torch.from_numpy(uv0)).cpu().numpy()
    one = psdr.Subdivision(box, levels=1)
    mid = one.refine_uv(torch.from_numpy(uv0))
    want, bound = _bounds(chain[0][0], uv0, False)
    _check(mid.cpu().numpy(), want, bound, "uv level 0")
    want, bound = _bounds(chain[1][0], mid.cpu().numpy(), False)
    _check(got, want, bound, "uv level 1")
    g = sub.restrict_uv(torch.ones(sub.num_uv_out, 1))
    assert abs(float(g.sum()) - sub.num_uv_out) <= 1e-3                 # the rows of S sum to 1: the columns' sums add up to the row count
    # the fine mesh carries the operator's topology, uv included
    fine = sub.to_mesh(sub.refine(torch.tensor(np.asarray(box.vertex_positions, np.float32))), sub.refine_uv(torch.from_numpy(uv0)))
    assert (int(fine.num_vertices), int(fine.num_faces)) == (sub.num_vertices_out, 16 * 12)
    assert np.array_equal(np.asarray(fine.face_indices).reshape(-1, 3), sub.faces)
    assert np.array_equal(np.asarray(fine.face_uv_indices).reshape(-1, 3), sub.face_uv)
    assert np.array_equal(np.asarray(fine.vertex_uv, np.float32).reshape(-1, 2), got)


def test_gradient_of_a_render_reaches_the_cage(psdr):
    """the scene of test_gradient_of_a_render_reaches_the_differential_coordinates: the ball's 642 vertices are S c, and c.grad = S^T v.grad"""
    import torch
    from psdr_jit_amd import Matrix4fC, Matrix4fD
    D = scenes.DATA
    sc = psdr.Scene()
    sc.opts.spp, sc.opts.sppe, sc.opts.sppse = 8, 8, 8
    sc.opts.width = sc.opts.height = 40
    sc.opts.log_level = 0
    cam = psdr.PerspectiveCamera(60, 0.000001, 10000000.)
    cam.to_world = Matrix4fD([[1., 0., 0., 278.], [0., 1., 0., 273.], [0., 0., 1., -500.], [0., 0., 0., 1.]])
    sc.add_Sensor(cam)
    sc.add_BSDF(psdr.DiffuseBSDF([0.0, 0.0, 0.0]), "light")
    sc.add_BSDF(psdr.DiffuseBSDF([0.9, 0.6, 0.1]), "ball")
    sc.add_BSDF(psdr.DiffuseBSDF([0.95, 0.95, 0.95]), "white")
    I = np.eye(4, dtype=np.float32).tolist()
    sc.add_Mesh(os.path.join(D, "cbox_luminaire.obj"), Matrix4fC([[1., 0., 0., 0.], [0., 1., 0., -0.5], [0., 0., 1., 0.], [0., 0., 0., 1.]]), "light", psdr.AreaLight([20.0, 20.0, 8.0]))
    cage = psdr.Mesh()
    cage.load(BALL)
    sub = psdr.Subdivision(cage, levels=1)
    assert (sub.num_vertices_in, sub.num_vertices_out, sub.faces.shape) == (162, 642, (1280, 3))
    c = torch.tensor(np.asarray(cage.vertex_positions, np.float32)).requires_grad_()
    v = sub.refine(c)
    v.retain_grad()
    ball = sub.to_mesh(v)
    assert (int(ball.num_vertices), int(ball.num_faces)) == (642, 1280)
    assert np.array_equal(np.asarray(ball.face_indices).reshape(-1, 3), sub.faces)
    sc.add_Mesh(ball, "ball", None)
    for f in ("cbox_floor", "cbox_back"):
        sc.add_Mesh(os.path.join(D, f + ".obj"), Matrix4fC(I), "white", None)
    sc.configure()
    sc.configure([0])
    img = psdr.PathTracer(2).renderD(sc, 0, seed=9)
    w = torch.linspace(0.5, 1.5, img.numel(), device=img.device).reshape(img.shape)
    (img * w).sum().backward()
    assert v.grad is not None and c.grad is not None
    gv = v.grad.cpu().numpy()
    assert np.isfinite(gv).all() and np.all(np.linalg.norm(gv.astype(np.float64), axis=0) > 0.0)
    faces = np.asarray(cage.face_indices).reshape(-1, 3)
    S64 = ref.reference_chain("ball", faces, 162, "loop", 1)[0][0]
    want, bound = _bounds(S64, gv, True)
    assert c.grad.device.type == "cpu" and tuple(c.grad.shape) == (162, 3)
    _check(c.grad.numpy(), want, bound, "c.grad")


def test_refusals(psdr):
    """every ValueError of the Python layer and every message of create's validation; nothing here reaches a kernel"""
    import ctypes as C
    import torch
    from psdr_jit_amd import cabi
    sub = _setup(psdr, "tetrahedron", "loop")[0][0]
    for call, arg in ((sub.refine, torch.zeros(5, 3)), (sub.refine, torch.zeros(4, 5)), (sub.refine, torch.zeros(4)), (sub.refine, torch.zeros(4, 0)),
                      (sub.refine, torch.zeros(4, 3, dtype=torch.int32)), (sub.restrict, torch.zeros(4, 3)), (sub.restrict, torch.zeros(10, 5)),
                      (sub.refine_uv, torch.zeros(4, 2)), (sub.restrict_uv, torch.zeros(10, 2)), (sub.to_mesh, torch.zeros(4, 3)), (sub.to_mesh, torch.zeros(10, 2))):
        with pytest.raises(ValueError):
            call(arg)
    with pytest.raises(ValueError, match="no uv"):
        sub.to_mesh(torch.zeros(10, 3), torch.zeros(10, 2))
    with pytest.raises(ValueError, match="no uv"):
        sub.csr(0, uv=True)
    with pytest.raises(ValueError, match="level"):
        sub.csr(1)
    with pytest.raises(ValueError, match="levels"):
        psdr.Subdivision(ref.TETRAHEDRON, 4, levels=0)
    with pytest.raises(ValueError, match="scheme"):
        psdr.Subdivision(ref.TETRAHEDRON, 4, scheme="sqrt3")
    with pytest.raises(ValueError, match="repeats"):
        psdr.Subdivision([[0, 1, 1]], 4)
    with pytest.raises(ValueError, match="outside"):
        psdr.Subdivision(ref.TETRAHEDRON, 3)
    with pytest.raises(ValueError, match="face_uv"):
        psdr.Subdivision(ref.TETRAHEDRON, 4, face_uv=ref.TETRAHEDRON[:3], num_uv=4)
    with pytest.raises(ValueError, match="num_vertices"):
        psdr.Subdivision(ref.TETRAHEDRON)

    # the C ABI, with deliberately malformed HOST arrays: create refuses them before any device call
    L = cabi.lib()
    good = [a.copy() for a in sub.csr(0)] + [a.copy() for a in sub.csr(0, transpose=True)]

    def create(n_in=4, n_out=10, edit=None, null=None):
        arrays = [a.copy() for a in good]
        if edit:
            edit(arrays)
        ptrs = [None if i == null else a.ctypes.data for i, a in enumerate(arrays)]
        h = C.c_void_p()
        rc = L.psdr_hip_subdiv_create(n_in, n_out, *ptrs, C.byref(h), None)
        msg = L.psdr_hip_last_error().decode() if rc else ""
        if not rc:
            L.psdr_hip_subdiv_destroy(h)
        return rc, msg

    assert create() == (0, "")

    def put(i, k, value):
        def edit(arrays):
            arrays[i][k] = value
        return edit

    cases = [(dict(edit=put(0, 3, 1)), "row_begin is not monotonic at row 2"),
             (dict(edit=put(3, 2, 0)), "t_row_begin is not monotonic at row 1"),
             (dict(edit=put(0, 0, 1)), "row_begin[0] = 1, must be 0"),
             (dict(edit=put(3, 0, 2)), "t_row_begin[0] = 2, must be 0"),
             (dict(edit=put(1, 5, 4)), "col[5] = 4 of row 1 is outside [0, 4)"),
             (dict(edit=put(1, 0, -1)), "col[0] = -1 of row 0 is outside [0, 4)"),
             (dict(edit=put(4, 7, 10)), "t_col[7] = 10 of row"),
             (dict(edit=put(2, 6, np.nan)), "weight[6] of row 1 is not finite"),
             (dict(edit=put(5, 1, np.inf)), "t_weight[1] of row 0 is not finite"),
             (dict(edit=put(3, 4, int(good[3][4]) - 1)), "the same number"),
             (dict(null=0), "row_begin is NULL"), (dict(null=1), "col is NULL"), (dict(null=5), "t_weight is NULL"),
             (dict(n_in=0), "must be positive"), (dict(n_out=-3), "must be positive"),
             (dict(n_out=2 ** 29), "below 2^31")]
    for kw, text in cases:
        rc, msg = create(**kw)
        print(kw.get("null", ""), msg)
        assert rc != 0 and msg.startswith("psdr_hip_subdiv_create: ") and text in msg, (kw, msg)
    assert L.psdr_hip_subdiv_create(4, 10, *[a.ctypes.data for a in good], None, None) != 0 and b"out is NULL" in L.psdr_hip_last_error()

    # apply / apply_adj: C = 5, NULL and aliased arrays return before anything is launched
    x, y = torch.zeros(4, 4, device="cuda"), torch.zeros(10, 4, device="cuda")
    hp = sub._handles[False][0].ptr
    for fn, name in ((L.psdr_hip_subdiv_apply, "psdr_hip_subdiv_apply"), (L.psdr_hip_subdiv_apply_adj, "psdr_hip_subdiv_apply_adj")):
        for Cn in (5, 0, -1):
            assert fn(hp, x.data_ptr(), Cn, y.data_ptr(), None) != 0
            assert L.psdr_hip_last_error().decode() == "%s: C = %d, must be in [1, 4]" % (name, Cn)
        assert fn(hp, None, 3, y.data_ptr(), None) != 0 and b"NULL" in L.psdr_hip_last_error()
        assert fn(hp, x.data_ptr(), 3, None, None) != 0 and b"NULL" in L.psdr_hip_last_error()
        assert fn(None, x.data_ptr(), 3, y.data_ptr(), None) != 0 and b"handle is NULL" in L.psdr_hip_last_error()
        assert fn(hp, y.data_ptr(), 3, y.data_ptr(), None) != 0 and b"different arrays" in L.psdr_hip_last_error()
    assert L.psdr_hip_subdiv_destroy(None) != 0
    torch.cuda.synchronize()
    assert torch.equal(y, torch.zeros_like(y))
