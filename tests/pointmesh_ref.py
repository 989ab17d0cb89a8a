"""An independent reading of the point-to-mesh distance (include/psdr_hip.h, THE POINT-TO-MESH DISTANCE, states the definition; psdr_jit_amd/pointmesh.py and
csrc/hip/pointmesh.hip implement it): numpy only, shares no code with the package.

pairs(P, A, B, C, dtype) is the pair function, broadcasting: Ericson's cascade in the definition's order - `np.where`s applied from the last region to the first, so that
the first test that holds decides - with every operation a numpy operation of `dtype`: one rounding each, the definition's order.  In float32 this is the kernel's
operation order: the kernel's per-face record holds a, ab = b - a, ac = c - a, b and c and nothing else is precomputed, so ab and ac are rounded once, from the vertices,
here as there.  closest() reduces it over all pairs to the two nearest-index arrays; closest_alt() is a second formulation in float64 that shares nothing with the
cascade: the projection onto the plane if it lies inside the face, else the minimum over the three clamped segments.

evaluate() gives the two direction means, the loss and the gradients through GIVEN indices (they are constants), with `dtype`'s own barycentrics of the given pairs and in
the definition's order of addition.  Its float32 form is the yardstick of the accuracy rule (tests/meshreg_ref.py says why it has this form):

    e_gpu = max |device - float64|,  e_32 = max |float32 checker - float64|,  G = max |float64|,  u = 2^-24:      e_gpu <= 4 max(e_32, u G)

Face indices are NOT compared for equality: a point nearest a shared edge or vertex is equally near several faces and the two precisions pick differently.  What is
compared is unique: the distances, the closest points, and the float64 distance of the face the device chose."""
import collections

import numpy as np

import subdiv_ref as sref

U = 2.0 ** -24
CHUNK = 1 << 20          # pairs per chunk

Closest = collections.namedtuple("Closest", ["face_of_point", "bary_p", "dist2_p", "region_p", "point_of_face", "bary_f", "dist2_f"])


def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def _quot(num, den):
    zero = den == 0
    return np.where(zero, num.dtype.type(0), num / np.where(zero, num.dtype.type(1), den))


def pairs(P, A, B, C, dtype=np.float64):
    """the pair function on broadcastable [..., 3] arrays -> (s, t, dist2, region 1 .. 7, e [..., 3]); every operation in `dtype`"""
    T = dtype
    P, A, B, C = (np.asarray(x).astype(T) for x in (P, A, B, C))
    ab, ac = B - A, C - A
    ap, bp, cp = P - A, P - B, P - C
    d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    d43, d56 = d4 - d3, d5 - d6
    zero, one = T(0), T(1)
    den = (va + vb) + vc
    s, t = _quot(vb, den), _quot(vc, den)
    region = np.full(s.shape, 7, np.int8)

    def put(cond, rs, rt, k):
        nonlocal s, t, region
        s, t, region = np.where(cond, rs, s), np.where(cond, rt, t), np.where(cond, np.int8(k), region)

    t6 = _quot(d43, d43 + d56)
    put((va <= 0) & (d43 >= 0) & (d56 >= 0), one - t6, t6, 6)
    put((vb <= 0) & (d2 >= 0) & (d6 <= 0), zero, _quot(d2, d2 - d6), 5)
    put((d6 >= 0) & (d5 <= d6), zero, one, 4)
    put((vc <= 0) & (d1 >= 0) & (d3 <= 0), _quot(d1, d1 - d3), zero, 3)
    put((d3 >= 0) & (d4 <= d3), one, zero, 2)
    put((d1 <= 0) & (d2 <= 0), zero, zero, 1)
    s, t = s.astype(T), t.astype(T)
    e = ap - (s[..., None] * ab + t[..., None] * ac)
    dist2 = _dot(e, e)
    assert dist2.dtype == T and e.dtype == T
    return s, t, dist2, region, e


def _corners(v, faces):
    v, f = np.asarray(v), np.asarray(faces, np.int64)
    return v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]


def matrix(p, v, faces, dtype=np.float64):
    """dist2 [N, F] over all pairs (small cases)"""
    A, B, C = _corners(v, faces)
    return pairs(np.asarray(p)[:, None, :], A[None], B[None], C[None], dtype)[2]


def bary_of(s, t):
    return np.stack([(s.dtype.type(1) - s) - t, s, t], -1)


def chosen(p, v, faces, point, face, dtype=np.float64):
    """the pairs (p[point[k]], faces[face[k]]) -> (bary [K, 3], dist2 [K], q [K, 3] = sum_c bary_c v_c in float64 from these barycentrics, e [K, 3])"""
    A, B, C = _corners(v, np.asarray(faces, np.int64)[np.asarray(face, np.int64)])
    s, t, d, _r, e = pairs(np.asarray(p)[np.asarray(point, np.int64)], A, B, C, dtype)
    bary = bary_of(s, t)
    b64 = bary.astype(np.float64)
    q = b64[:, 0:1] * A.astype(np.float64) + b64[:, 1:2] * B.astype(np.float64) + b64[:, 2:3] * C.astype(np.float64)
    return bary, d, q, e


def closest(p, v, faces, dtype=np.float64):
    """the cascade over all pairs, reduced: a Closest.  argmin returns the first (lowest) index of the minimum, and so does the running `<` over the row chunks"""
    p, F = np.asarray(p), len(faces)
    N = len(p)
    A, B, C = _corners(v, faces)
    fop, sp, tp, dp, rp = np.empty(N, np.int32), np.empty(N, dtype), np.empty(N, dtype), np.empty(N, dtype), np.empty(N, np.int8)
    pof, sf, tf, df = np.zeros(F, np.int32), np.zeros(F, dtype), np.zeros(F, dtype), np.full(F, np.inf, dtype)
    rows = max(1, CHUNK // F)
    for r0 in range(0, N, rows):
        s, t, d, reg, _e = pairs(p[r0:r0 + rows, None, :], A[None], B[None], C[None], dtype)
        k, at = d.argmin(1), np.arange(d.shape[0])
        fop[r0:r0 + rows], sp[r0:r0 + rows], tp[r0:r0 + rows], dp[r0:r0 + rows], rp[r0:r0 + rows] = k, s[at, k], t[at, k], d[at, k], reg[at, k]
        k, at = d.argmin(0), np.arange(F)
        better = d[k, at] < df
        pof, sf, tf, df = np.where(better, k + r0, pof).astype(np.int32), np.where(better, s[k, at], sf), np.where(better, t[k, at], tf), np.where(better, d[k, at], df)
    return Closest(fop, bary_of(sp, tp), dp, rp, pof, bary_of(sf, tf), df)


def closest_from_matrix(p, v, faces, d, dtype):
    """a Closest (region_p left None) from the dist2 matrix `d` [N, F] of these very inputs in `dtype`: argmin, then the winners' barycentrics by the pair function"""
    N, F = d.shape
    a, b = d.argmin(1).astype(np.int32), d.argmin(0).astype(np.int32)
    bp, dp, _q, _e = chosen(p, v, faces, np.arange(N), a, dtype)
    bf, df, _q, _e = chosen(p, v, faces, b, np.arange(F), dtype)
    assert np.array_equal(dp, d[np.arange(N), a]) and np.array_equal(df, d[b, np.arange(F)])
    return Closest(a, bp, dp, None, b, bf, df)


def closest_alt(p, v, faces):
    """a second float64 formulation over all pairs -> (dist2 [N, F], q [N, F, 3]): the foot of the perpendicular on the face's plane when it lies inside the face (three
    edge-side tests against the normal), else the nearest of the three clamped segment projections.  A face of zero area has no plane: the segments decide."""
    P = np.asarray(p, np.float64)[:, None, :]
    A, B, C = (x.astype(np.float64)[None] for x in _corners(v, faces))
    n = np.cross(B - A, C - A)
    nn = (n * n).sum(-1)
    ok = nn > 0
    safe = np.where(ok, nn, 1.0)
    foot = P - (((P - A) * n).sum(-1) / safe)[..., None] * n
    inside = ok
    for X, Y in ((A, B), (B, C), (C, A)):
        inside = inside & ((np.cross(Y - X, foot - X) * n).sum(-1) >= 0)
    best_d = np.full(inside.shape, np.inf)
    best_q = np.zeros(inside.shape + (3,))
    for X, Y in ((A, B), (B, C), (C, A)):
        d = Y - X
        dd = (d * d).sum(-1)
        u = np.clip(((P - X) * d).sum(-1) / np.where(dd > 0, dd, 1.0), 0.0, 1.0)
        u = np.where(dd > 0, u, 0.0)
        q = X + u[..., None] * d
        dist = ((P - q) ** 2).sum(-1)
        better = dist < best_d
        best_d, best_q = np.where(better, dist, best_d), np.where(better[..., None], q, best_q)
    dist_in = ((P - foot) ** 2).sum(-1)
    return np.where(inside, dist_in, best_d), np.where(inside[..., None], foot, best_q)


def _means(val, n, T):
    return T(val.sum() / T(n))


def evaluate(p, v, faces, face_of_point, point_of_face, weights=(1.0, 1.0), squared=True, dtype=np.float64):
    """-> {"terms": (mean_p, mean_f), "loss", "gp" [N, 3], "gv" [n, 3]} through the given indices, every operation in `dtype`; a direction of weight 0 (or whose indices
    are None) is left out and reports 0.  The orders of addition are the definition's: a point adds its own pair, then the sum (from 0) over the faces that chose it in
    ascending f; a face corner its own pair, then the sum (from 0) over the points that chose the face in ascending i; a vertex its corners in ascending (face, corner)
    order from 0."""
    T = dtype
    p, v, f = np.asarray(p), np.asarray(v), np.asarray(faces, np.int64)
    N, F, n = len(p), len(f), len(v)

    def direction(point, face, w, count):
        """the pairs (point[k], face[k]) -> (rho values, k r [K, 3], corner terms [K, 3, 3])"""
        bary, d, _q, e = chosen(p, v, f, point, face, T)
        if squared:
            val, k = d, np.full(len(d), T(2.0 * w / count))
        else:
            val = np.sqrt(d)
            pos = d > 0
            k = np.where(pos, T(1.0 * w / count) / np.where(pos, val, T(1)), T(0)).astype(T)
        kr = k[:, None] * e
        return val, kr, -(kr[:, None, :] * bary[:, :, None])

    terms, loss = [T(0), T(0)], None
    gp_own = gp_sum = c_own = c_sum = None
    if weights[0] > 0 and face_of_point is not None:
        a = np.asarray(face_of_point, np.int64)
        val, kr, ct = direction(np.arange(N), a, weights[0], N)
        terms[0] = _means(val, N, T)
        loss = T(weights[0]) * terms[0]
        gp_own = kr
        c_sum = np.zeros((F, 3, 3), T)
        np.add.at(c_sum, a, ct)                         # in ascending point order
    if weights[1] > 0 and point_of_face is not None:
        b = np.asarray(point_of_face, np.int64)
        val, kr, ct = direction(b, np.arange(F), weights[1], F)
        terms[1] = _means(val, F, T)
        loss = T(weights[1]) * terms[1] if loss is None else loss + T(weights[1]) * terms[1]
        c_own = ct
        gp_sum = np.zeros((N, 3), T)
        np.add.at(gp_sum, b, kr)                        # in ascending face order
    zero_p, zero_c = np.zeros((N, 3), T), np.zeros((F, 3, 3), T)
    gp = zero_p if gp_own is None and gp_sum is None else gp_sum if gp_own is None else gp_own if gp_sum is None else gp_own + gp_sum
    corners = zero_c if c_own is None and c_sum is None else c_sum if c_own is None else c_own if c_sum is None else c_own + c_sum
    gv = np.zeros((n, 3), T)
    np.add.at(gv, f.reshape(-1), corners.reshape(-1, 3))
    return {"terms": tuple(terms), "loss": T(0) if loss is None else T(loss), "gp": gp.astype(T), "gv": gv}


def ratio(dev, f32, f64):
    """e_gpu / max(e_32, u G) (0 when everything is exactly 0), and its parts"""
    dev, f32, f64 = (np.asarray(a, np.float64) for a in (dev, f32, f64))
    e_gpu, e_32, G = np.abs(dev - f64).max(), np.abs(f32 - f64).max(), np.abs(f64).max()
    yard = max(e_32, U * G)
    return (0.0 if e_gpu == 0 else e_gpu / yard if yard > 0 else np.inf), e_gpu, e_32, G


# ---- the inputs

def _uniform(n, seed, lo=-1.0, hi=1.0):
    return np.random.default_rng(seed).uniform(lo, hi, (n, 3)).astype(np.float32)


_BUNNY = []


def bunny():
    """the bunny's vertices scaled into the unit cube, float32 [2503, 3], and its faces"""
    if not _BUNNY:
        f, n, v, _ft, _vt = sref.load_obj(sref.BUNNY)
        v = (v - v.min(0)) / (v.max(0) - v.min(0)).max()
        _BUNNY.append((v.astype(np.float32), np.array(f, np.int64)))
    return _BUNNY[0]


def lattice(num_faces):
    """the first num_faces triangles of a height field over a grid: well shaped, and the height's curvature leaves no two neighbours coplanar -> (v float32, faces)"""
    k = 2
    while 2 * k * k < num_faces:
        k += 1
    x, y = np.meshgrid(np.arange(k + 1) / k, np.arange(k + 1) / k, indexing="ij")
    z = 0.25 * np.sin(3.1 * x + 0.4) * np.cos(2.3 * y - 0.2) + 0.15 * x * y
    v = np.stack([x, y, z], -1).reshape(-1, 3).astype(np.float32)
    i, j = (a.reshape(-1) for a in np.meshgrid(np.arange(k), np.arange(k), indexing="ij"))
    c = i * (k + 1) + j                              # the cell's corner (i, j); per cell the two triangles, cells in row-major order
    faces = np.stack([np.stack([c, c + k + 1, c + 1], 1), np.stack([c + k + 1, c + k + 2, c + 1], 1)], 1).reshape(-1, 3)
    return v, np.ascontiguousarray(faces[:num_faces], np.int64)


def degenerate_mesh():
    """proper faces, a face of zero area (three distinct collinear vertices), a face with an edge of zero length (two ids at one position, the face's b and c) and a sliver
    of aspect 1 : 4000.  On these the cascade still returns the closest point (closest_alt agrees); a face whose a and b coincide is the one arrangement where it does not -
    test_pointmesh_cpu.py states what it returns there"""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.3], [0.5, 0.5, 1.0],            # 0 .. 4: a small proper patch
                  [2, 0, 0], [2.5, 0, 0], [3, 0, 0],                                          # 5 .. 7: collinear
                  [0, 2, 0], [0, 2, 0], [1, 2, 0.5],                                          # 8, 9: one position under two ids
                  [2, 2, 0], [3, 2, 0], [2.5, 2.00025, 0]], np.float64)                       # 11 .. 13: the sliver
    faces = np.array([[0, 1, 2], [1, 3, 2], [0, 4, 1], [2, 4, 0], [1, 4, 3], [3, 4, 2],
                      [5, 6, 7], [10, 8, 9], [11, 12, 13]], np.int64)
    return v.astype(np.float32), faces


def case(name):
    """(p, v, faces) float32 / int64 of a named case"""
    if name == "regions":                           # uniform points in the bunny's bounding box enlarged by 20 % per side: every region wins often
        v, f = bunny()
        lo, hi = v.min(0), v.max(0)
        pad = 0.2 * (hi - lo)
        r = np.random.default_rng(41)
        return r.uniform(lo - pad, hi + pad, (1000, 3)).astype(np.float32), v, f
    if name == "near":                              # points within 2 % of the bunny's surface: the winners are interior
        v, f = bunny()
        r = np.random.default_rng(42)
        k = r.integers(0, len(f), 800)
        w = r.dirichlet((1.0, 1.0, 1.0), 800)
        q = (w[:, :, None] * v[f[k]].astype(np.float64)).sum(1)
        return (q + r.normal(0.0, 0.01, q.shape)).astype(np.float32), v, f
    if name == "degenerate":
        v, f = degenerate_mesh()
        r = np.random.default_rng(43)
        p = np.concatenate([r.uniform(-0.5, 3.5, (400, 3)) * (1, 1, 0.4), v.astype(np.float64), v[f].astype(np.float64).mean(1)])
        return p.astype(np.float32), v, f
    raise KeyError(name)


CASES = ("regions", "near", "degenerate")

_REF = {}


def reference(name):
    """(p, v, faces, Closest in float64, Closest in float32) of a named case, computed once and shared (do not modify)"""
    if name not in _REF:
        p, v, f = case(name)
        _REF[name] = (p, v, f, closest(p, v, f, np.float64), closest(p, v, f, np.float32))
    return _REF[name]


def sweep_reference(max_points, max_faces):
    """the plan-boundary sweep: one lattice, one cloud, the full float64 and float32 dist2 matrices [max_points, max_faces] - every (N, F) of the sweep is a leading block"""
    key = ("sweep", max_points, max_faces)
    if key not in _REF:
        v, f = lattice(max_faces)
        p = (_uniform(max_points, 44, -0.2, 1.2) * np.float32([1, 1, 0.5])).astype(np.float32)
        _REF[key] = (p, v, f, matrix(p, v, f, np.float64), matrix(p, v, f, np.float32))
    return _REF[key]
