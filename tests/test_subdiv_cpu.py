"""CPU tests of the subdivision topology (psdr_jit_amd/subdiv.py: subdivision_level), loaded by path: it needs neither a GPU nor the native library.

The matrix S, its transpose, the fine faces and the counts are checked against tests/subdiv_ref.py - an independent per-face Python loop over
dictionaries in float64 - and against answers written out here: the tetrahedron's ten rows, the `bowtie` and `book` matrices, the figures of the
repository's meshes.

The figures of bunny_low.obj "after two levels" (39 826 vertices, 79 488 faces, 84 sharp edges) are read as: the vertex and face counts are those of
the mesh the second level returns, and 84 is the sharp-edge count the second level itself found, i.e. of the once-refined mesh it was built from
(42 doubled once).  The twice-refined mesh has 168; test_counts checks that too, by enumerating its edges."""
import importlib.util
import os

import numpy as np
import pytest

import subdiv_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24


def _load():
    spec = importlib.util.spec_from_file_location("_psdr_subdiv_t", os.path.join(ROOT, "psdr_jit_amd", "subdiv.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


subdiv = _load()

_OBJ = {}


def _mesh(name):
    """(faces, n, float64 positions or None)"""
    if name == "tetrahedron":
        return ref.TETRAHEDRON, 4, 16.0 * np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float64)
    if name == "bowtie":
        return ref.BOWTIE, 5, np.array([[0, 0, 0], [1, 1, 0], [1, -1, .5], [-1, -1, 0], [-1, 1, .25]], np.float64)
    if name == "book":
        return ref.BOOK, 5, np.array([[0, 0, 0], [0, 0, 1], [1, 0, .5], [-1, 1, .5], [-1, -1, .25]], np.float64)
    if name == "grid9":
        f, n = ref.grid(9)
        ij = np.stack(np.meshgrid(np.arange(9.), np.arange(9.), indexing="ij"), -1).reshape(-1, 2)
        return f, n, np.concatenate([ij, np.sin(ij[:, :1]) * np.cos(ij[:, 1:])], 1)
    if name == "fan":
        f, n = ref.fan(200)
        t = 2 * np.pi * np.arange(200) / 200
        return f, n, np.concatenate([[[0, 0, 1.]], np.stack([np.cos(t), np.sin(t), 0 * t], 1), [[5., 5., 5.]]])
    if name not in _OBJ:
        path = ref.BUNNY if name == "bunny" else os.path.join(ref.CBOX, "cbox_%s.obj" % name)
        _OBJ[name] = ref.load_obj(path)
    f, n, v, _fuv, _uv = _OBJ[name]
    return f, n, v


MESHES = ["bunny", "smallball", "largebox", "floor", "grid9", "tetrahedron", "bowtie", "book", "fan"]
#              V     F     E     sharp
TABLE = {"bunny": (2503, 4968, 7473, 42), "smallball": (162, 320, 480, 0), "largebox": (8, 12, 18, 0), "floor": (12, 2, 5, 4)}


def _edges(faces):
    """{undirected edge: number of faces at it}, by a plain loop"""
    count = {}
    for a, b, c in np.asarray(faces).tolist():
        for p, q in ((a, b), (b, c), (c, a)):
            count[(min(p, q), max(p, q))] = count.get((min(p, q), max(p, q)), 0) + 1
    return count


def _dense_rows(lv, transpose=False):
    rb, col, w = (lv.t_row_begin, lv.t_col, lv.t_weight) if transpose else (lv.row_begin, lv.col, lv.weight)
    return [(col[rb[i]:rb[i + 1]], w[rb[i]:rb[i + 1]]) for i in range(len(rb) - 1)]


_CHAIN = {}


def _chain(name, scheme, levels=2):
    """[SubdivisionLevel] per level, built once"""
    k = (name, scheme, levels)
    if k not in _CHAIN:
        f, n, _v = _mesh(name)
        out = []
        for _ in range(levels):
            out.append(subdiv.subdivision_level(np.asarray(f), n, scheme))
            f, n = out[-1].faces, out[-1].num_vertices_out
        _CHAIN[k] = out
    return _CHAIN[k]


@pytest.mark.parametrize("name", MESHES)
def test_counts(name):
    faces, n, _v = _mesh(name)
    F = len(faces)
    lv1, lv2 = _chain(name, "loop")
    e0 = _edges(faces)
    E, sharp = len(e0), sum(1 for m in e0.values() if m != 2)
    if name in TABLE:
        assert (n, F, E, sharp) == TABLE[name]
    assert (lv1.num_vertices_in, lv1.num_edges, lv1.num_sharp_edges) == (n, E, sharp)
    assert lv1.num_vertices_out == n + E and lv1.faces.shape == (4 * F, 3) and lv1.faces.dtype == np.int32
    e1 = _edges(lv1.faces)
    assert len(e1) == 2 * E + 3 * F
    assert (lv2.num_vertices_in, lv2.num_edges) == (n + E, len(e1))
    assert lv2.num_vertices_out == n + E + len(e1) and lv2.faces.shape == (16 * F, 3)
    # V - E + F is unchanged from level to level, the sharp-edge count doubles per level
    e2 = _edges(lv2.faces)
    chi = [n - E + F, lv1.num_vertices_out - len(e1) + 4 * F, lv2.num_vertices_out - len(e2) + 16 * F]
    assert chi[0] == chi[1] == chi[2]
    assert lv2.num_sharp_edges == 2 * sharp == sum(1 for m in e1.values() if m != 2)
    assert sum(1 for m in e2.values() if m != 2) == 4 * sharp
    if name == "bunny":
        assert (lv2.num_vertices_out, lv2.faces.shape[0], lv2.num_sharp_edges) == (39826, 79488, 84)
    if name == "floor":
        assert lv1.num_vertices_out == 17
        assert sum(1 for i in range(n) if not any(i in t for t in faces)) >= 2          # several vertices no face uses: identity rows
    if name == "fan":
        # the hub is smooth (200 interior spokes), every rim vertex a crease (two boundary edges): the hub's column holds itself and the 200 spokes
        assert n == 202 and len(_dense_rows(lv1)[0][0]) == 201 and len(_dense_rows(lv1, True)[0][0]) == 201
    # the linear scheme has the same topology
    ll = _chain(name, "linear")
    assert np.array_equal(ll[0].faces, lv1.faces) and np.array_equal(ll[1].faces, lv2.faces)


@pytest.mark.parametrize("scheme", ["loop", "linear"])
@pytest.mark.parametrize("name", MESHES)
def test_matrix_against_the_reference(name, scheme):
    faces, n, _v = _mesh(name)
    f = [list(t) for t in np.asarray(faces).tolist()]
    for lv in _chain(name, scheme):
        rows, fine, E, sharp = ref.reference_level(f, n, scheme)
        assert (lv.num_edges, lv.num_sharp_edges, lv.num_vertices_out) == (E, sharp, n + E)
        assert np.array_equal(lv.faces, np.array(fine))
        assert lv.weight.dtype == np.float32 and lv.col.dtype == np.int32 and lv.row_begin.dtype == np.int32
        assert lv.row_begin[0] == 0 and lv.row_begin[-1] == len(lv.col) == len(lv.weight) and len(lv.row_begin) == n + E + 1
        got = _dense_rows(lv)
        assert len(got) == len(rows)
        for i, ((col, w), want) in enumerate(zip(got, rows)):
            assert col.tolist() == sorted(want), (i, col, want)                 # the pattern, in ascending column order
            w64 = np.array([want[j] for j in col.tolist()])
            assert np.all(np.abs(w.astype(np.float64) - w64) <= 2 * np.spacing(w64.astype(np.float32)).astype(np.float64)), (i, w, w64)
            assert np.all(w >= 0)
            assert abs(float(w.astype(np.float64).sum()) - 1.0) <= 4 * U, (i, w)
        f, n = fine, n + E


@pytest.mark.parametrize("scheme", ["loop", "linear"])
@pytest.mark.parametrize("name", MESHES)
def test_transpose_holds_the_same_entries(name, scheme):
    for lv in _chain(name, scheme):
        assert lv.t_weight.dtype == np.float32 and lv.t_col.dtype == np.int32
        assert len(lv.t_row_begin) == lv.num_vertices_in + 1 and lv.t_row_begin[0] == 0
        assert lv.t_row_begin[-1] == len(lv.t_col) == len(lv.t_weight) == len(lv.weight)
        fwd = {}
        for i, (col, w) in enumerate(_dense_rows(lv)):
            for j, x in zip(col.tolist(), w.view(np.uint32).tolist()):
                assert (i, j) not in fwd
                fwd[(i, j)] = x
        seen = 0
        for j, (col, w) in enumerate(_dense_rows(lv, True)):
            assert np.all(np.diff(col) > 0), j                                   # ascending, so no entry twice
            for i, x in zip(col.tolist(), w.view(np.uint32).tolist()):
                assert fwd[(i, j)] == x, (i, j)
                seen += 1
        assert seen == len(fwd)


def _apply64(lv, x):
    y = np.zeros((lv.num_vertices_out,) + x.shape[1:])
    w = lv.weight.astype(np.float64)
    for i in range(lv.num_vertices_out):
        b0, b1 = lv.row_begin[i], lv.row_begin[i + 1]
        y[i] = w[b0:b1] @ x[lv.col[b0:b1]]
    return y


def test_tetrahedron_rows_are_the_known_answer():
    _f, _n, v = _mesh("tetrahedron")
    lv = _chain("tetrahedron", "loop")[0]
    want = [(3, 3, 3), (7, 3, 3), (3, 7, 3), (3, 3, 7), (6, 2, 2), (2, 6, 2), (2, 2, 6), (6, 6, 2), (6, 2, 6), (2, 6, 6)]
    got32 = np.zeros((10, 3), np.float32)
    for i, (col, w) in enumerate(_dense_rows(lv)):
        acc = np.zeros(3, np.float32)
        for j, x in zip(col, w):
            acc = acc + x * v[j].astype(np.float32)                              # every product and sum is exact: dyadic weights, small integers
        got32[i] = acc
    assert got32.tolist() == [list(map(float, t)) for t in want]


def _dense(lv):
    S = np.zeros((lv.num_vertices_out, lv.num_vertices_in))
    for i, (col, w) in enumerate(_dense_rows(lv)):
        S[i, col] = w
    return S


def test_bowtie_and_book_matrices():
    # bowtie: edges (0,1) (0,2) (0,3) (0,4) (1,2) (3,4), all boundary.  0 has four sharp edges: a corner.  1, 2, 3, 4 are creases.
    want = np.zeros((11, 5))
    want[0, 0] = 1
    want[1, [1, 0, 2]] = .75, .125, .125
    want[2, [2, 0, 1]] = .75, .125, .125
    want[3, [3, 0, 4]] = .75, .125, .125
    want[4, [4, 0, 3]] = .75, .125, .125
    for e, (a, b) in enumerate([(0, 1), (0, 2), (0, 3), (0, 4), (1, 2), (3, 4)]):
        want[5 + e, [a, b]] = .5
    lv = _chain("bowtie", "loop")[0]
    assert (lv.num_edges, lv.num_sharp_edges) == (6, 6)
    assert np.array_equal(_dense(lv), want)
    # book: edges (0,1) [three faces: sharp] (0,2) (0,3) (0,4) (1,2) (1,3) (1,4) [boundary].  0 and 1 have four sharp edges: corners.
    # 2, 3, 4 are creases over their two boundary edges, to 0 and to 1.
    want = np.zeros((12, 5))
    want[0, 0] = want[1, 1] = 1
    for v in (2, 3, 4):
        want[v, [v, 0, 1]] = .75, .125, .125
    for e, (a, b) in enumerate([(0, 1), (0, 2), (0, 3), (0, 4), (1, 2), (1, 3), (1, 4)]):
        want[5 + e, [a, b]] = .5
    lv = _chain("book", "loop")[0]
    assert (lv.num_edges, lv.num_sharp_edges) == (7, 7)
    assert np.array_equal(_dense(lv), want)


def _normals(v, f):
    f = np.asarray(f)
    return np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])


@pytest.mark.parametrize("name", ["bunny", "largebox", "grid9", "book"])
def test_fine_faces_keep_order_orientation_and_area(name):
    faces, n, v = _mesh(name)
    lv = _chain(name, "linear")[0]
    f = np.asarray(faces)
    num = {e: i for i, e in enumerate(sorted(_edges(faces)))}
    mid = lambda p, q: n + num[(min(p, q), max(p, q))]
    for k in (0, len(f) // 2, len(f) - 1):
        a, b, c = f[k].tolist()
        ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
        assert lv.faces[4 * k:4 * k + 4].tolist() == [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
    fine_v = _apply64(lv, v)
    assert np.array_equal(fine_v[:n], v)
    N0, N1 = _normals(v, f), _normals(fine_v, lv.faces)
    cos = (N1 * np.repeat(N0, 4, axis=0)).sum(1) / (np.linalg.norm(N1, axis=1) * np.repeat(np.linalg.norm(N0, axis=1), 4))
    assert cos.min() >= 1 - 1e-12
    A0, A1 = 0.5 * np.linalg.norm(N0, axis=1).sum(), 0.5 * np.linalg.norm(N1, axis=1).sum()
    print(name, "area", repr(A0), repr(A1))
    assert abs(A1 - A0) <= 1e-12 * A0


@pytest.mark.parametrize("scheme", ["loop", "linear"])
@pytest.mark.parametrize("name", ["bunny", "floor", "fan", "bowtie"])
def test_affine_invariance(name, scheme):
    _f, _n, v = _mesh(name)
    lv = _chain(name, scheme)[0]
    rng = np.random.default_rng(3)
    A, t = rng.standard_normal((3, 3)), rng.standard_normal(3)
    # in float64 with the float32 weights a row sums to 1 only within 4 * 2^-24: the exact statement is for the row-normalised weights
    S1 = _apply64(lv, np.ones((lv.num_vertices_in, 1)))
    lhs, rhs = _apply64(lv, v @ A + t) / S1, (_apply64(lv, v) / S1) @ A + t
    scale = np.abs(rhs).max()
    assert np.abs(lhs - rhs).max() <= 1e-12 * scale
    if scheme == "linear":          # 1 and 1/2 + 1/2: the rows sum to 1 exactly and the statement holds as it stands
        assert np.all(S1 == 1.0)
        assert np.abs(_apply64(lv, v @ A + t) - (_apply64(lv, v) @ A + t)).max() <= 1e-12 * scale


def test_uv_of_every_child_corner_is_the_parents_interpolation():
    faces, n, _v, fuv, uv = ref.load_obj(os.path.join(ref.CBOX, "cbox_largebox.obj"))
    assert fuv is not None and len(uv) == 21
    pos = subdiv.subdivision_level(np.asarray(faces), n, "loop")
    tex = subdiv.subdivision_level(np.asarray(fuv), len(uv), "linear")
    fine_uv = _apply64(tex, uv)
    # child k's corners in the parent's barycentric coordinates, in the specified child order (a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)
    h = 0.5
    bary = np.array([[[1, 0, 0], [h, h, 0], [h, 0, h]], [[0, 1, 0], [0, h, h], [h, h, 0]], [[0, 0, 1], [h, 0, h], [0, h, h]], [[h, h, 0], [0, h, h], [h, 0, h]]])
    for f in range(len(faces)):
        parent = uv[np.asarray(fuv[f])]
        for k in range(4):
            assert np.abs(fine_uv[tex.faces[4 * f + k]] - bary[k] @ parent).max() <= 1e-15, (f, k)
            # ... and the position indices of the same child name the same corners of the same parent
            for corner in range(3):
                i = pos.faces[4 * f + k][corner]
                assert (i < n) == (tex.faces[4 * f + k][corner] < len(uv))
                if i < n:
                    assert i == faces[f][int(np.argmax(bary[k][corner]))]


def test_errors():
    f = np.array(ref.TETRAHEDRON)
    with pytest.raises(ValueError, match="repeats"):
        subdiv.subdivision_level(np.array([[0, 1, 2], [1, 1, 3]]), 4, "loop")
    with pytest.raises(ValueError, match="outside"):
        subdiv.subdivision_level(f, 3, "loop")
    with pytest.raises(ValueError, match="outside"):
        subdiv.subdivision_level(np.array([[0, 1, -1]]), 4, "loop")
    with pytest.raises(ValueError, match="scheme"):
        subdiv.subdivision_level(f, 4, "butterfly")
    with pytest.raises(ValueError, match=r"\[f, 3\]"):
        subdiv.subdivision_level(f.reshape(-1), 4, "loop")
    # the class checks its arguments before it touches the device
    with pytest.raises(ValueError, match="levels"):
        subdiv.Subdivision(f, 4, levels=0)
    with pytest.raises(ValueError, match="scheme"):
        subdiv.Subdivision(f, 4, scheme="butterfly")
    with pytest.raises(ValueError, match="face_uv"):
        subdiv.Subdivision(f, 4, face_uv=f[:3], num_uv=4)
    with pytest.raises(ValueError, match="num_vertices"):
        subdiv.Subdivision(f)
    with pytest.raises(ValueError, match="repeats"):
        subdiv.Subdivision(f, 4, face_uv=np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 3]]), num_uv=4)
    with pytest.raises(ValueError, match="outside"):
        subdiv.Subdivision(f, 4, face_uv=f, num_uv=3)
