"""An independent reading of the signed distance (include/psdr_hip.h, THE SIGNED DISTANCE, states the definition; psdr_jit_amd/sdf.py and csrc/hip/sdf.hip implement it):
numpy only, shares no code with the package.  The magnitude - nearest face, barycentrics, dist2 - is tests/pointmesh_ref.py's.

theta(P, A, B, C, dtype) is the pair function, broadcasting: Van Oosterom & Strackee's half solid angle with every operation a numpy operation of `dtype`, in the definition's
order, 0 where Nm == 0.  winding() sums it over the faces in ascending f, sequentially (a cumulative sum, not numpy's pairwise one), in `dtype`, and also returns
sum_f |theta| / (2 pi): the magnitude G of the accuracy rule (tests/meshreg_ref.py says why the rule has this form):

    e_gpu = max |device - float64|,  e_32 = max |float32 checker - float64|,  u = 2^-24:      e_gpu <= 4 max(e_32, u G)

signed() is s = -+ sqrt(D_p) with the sign of `dtype`'s own winding number; vjp() the vector-Jacobian product of s through GIVEN indices and a GIVEN sign (they are constants),
with `dtype`'s own barycentrics of the given pairs and in the definition's orders of addition.

The meshes: an octahedron, two overlapping cubes (w = 2 in the overlap), the bunny (42 boundary edges), pointmesh_ref's lattice as the open mesh, and an irregular octahedron
with a face of zero area and a face over a repeated position; reversed() gives any of them with the other winding."""
import numpy as np

import pointmesh_ref as pref

U = pref.U
CHUNK = pref.CHUNK


def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def theta(P, A, B, C, dtype=np.float64):
    """the pair function on broadcastable [..., 3] arrays; every operation in `dtype`"""
    T = dtype
    P, A, B, C = (np.asarray(x).astype(T) for x in (P, A, B, C))
    a, b, c = A - P, B - P, C - P
    la, lb, lc = np.sqrt(_dot(a, a)), np.sqrt(_dot(b, b)), np.sqrt(_dot(c, c))
    n = np.stack([b[..., 1] * c[..., 2] - b[..., 2] * c[..., 1], b[..., 2] * c[..., 0] - b[..., 0] * c[..., 2], b[..., 0] * c[..., 1] - b[..., 1] * c[..., 0]], -1)
    nm = _dot(a, n)
    dn = ((la * lb) * lc + _dot(a, b) * lc) + (_dot(b, c) * la + _dot(c, a) * lb)
    th = np.where(nm == 0, T(0), np.arctan2(nm, dn))
    assert th.dtype == T
    return th


def theta_matrix(p, v, faces, dtype=np.float64):
    """theta [N, F] over all pairs (small cases)"""
    A, B, C = pref._corners(v, faces)
    return theta(np.asarray(p)[:, None, :], A[None], B[None], C[None], dtype)


def from_matrix(th):
    """(w [N, F], G [N, F]) of every leading block of faces: column F - 1 holds the sums over the first F faces, added in ascending f in th's dtype"""
    T = th.dtype.type
    return np.cumsum(th, axis=1, dtype=T) * T(1.0 / (2.0 * np.pi)), np.cumsum(np.abs(th.astype(np.float64)), axis=1) / (2.0 * np.pi)


def winding(p, v, faces, dtype=np.float64):
    """-> (w [N] in `dtype`, G [N] float64 = sum_f |theta| / (2 pi))"""
    p = np.asarray(p)
    N, F = len(p), len(faces)
    w, G = np.empty(N, dtype), np.empty(N, np.float64)
    rows = max(1, CHUNK // F)
    for r0 in range(0, N, rows):
        wm, gm = from_matrix(theta_matrix(p[r0:r0 + rows], v, faces, dtype))
        w[r0:r0 + rows], G[r0:r0 + rows] = wm[:, -1], gm[:, -1]
    return w, G


def inside_of(w, orientation=1):
    return np.asarray(w).dtype.type(orientation) * np.asarray(w) > 0.5


def signed(dist2, inside):
    d = np.sqrt(np.asarray(dist2))
    return np.where(inside, -d, d).astype(d.dtype)


def vjp(p, v, faces, face, inside, g, dtype=np.float64):
    """the vector-Jacobian product of s through the given indices and sign -> (s [N], gp [N, 3], gv [n, 3]), every operation in `dtype`: k_i = g_i / s_i (0 where s_i == 0),
    p_i receives k_i r_i, corner c of face[i] receives -((k_i r_i) bary_ic); a face's corner record adds the points that chose it in ascending i from 0, a vertex its corners in
    ascending (face, corner) order from 0"""
    T = dtype
    p, v, f = np.asarray(p), np.asarray(v), np.asarray(faces, np.int64)
    N, F, n = len(p), len(f), len(v)
    a = np.asarray(face, np.int64)
    bary, d, _q, e = pref.chosen(p, v, f, np.arange(N), a, T)
    s = signed(d, np.asarray(inside, bool))
    zero = s == 0
    k = np.where(zero, T(0), np.asarray(g).astype(T) / np.where(zero, T(1), s)).astype(T)
    kr = k[:, None] * e
    corners = np.zeros((F, 3, 3), T)
    np.add.at(corners, a, -(kr[:, None, :] * bary[:, :, None]))          # in ascending point order
    gv = np.zeros((n, 3), T)
    np.add.at(gv, f.reshape(-1), corners.reshape(-1, 3))
    assert kr.dtype == T and gv.dtype == T
    return s, kr, gv


def ratio(dev, f32, f64, G=None):
    """e_gpu / max(e_32, u G) (0 when everything is exactly 0), and its parts; G defaults to max |float64|"""
    dev, f32, f64 = (np.asarray(a, np.float64) for a in (dev, f32, f64))
    e_gpu, e_32 = np.abs(dev - f64).max(), np.abs(f32 - f64).max()
    G = np.abs(f64).max() if G is None else float(np.max(G))
    yard = max(e_32, U * G)
    return (0.0 if e_gpu == 0 else e_gpu / yard if yard > 0 else np.inf), e_gpu, e_32, G


# ---- the meshes

def reversed_faces(faces):
    """every face with the other winding"""
    return np.ascontiguousarray(np.asarray(faces, np.int64)[:, [0, 2, 1]])


def _outward(v, faces, centre):
    """the faces wound counter-clockwise seen from outside the convex solid around `centre`"""
    v, f = np.asarray(v, np.float64), np.asarray(faces, np.int64).copy()
    A, B, C = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    flip = (np.cross(B - A, C - A) * ((A + B + C) / 3.0 - centre)).sum(1) < 0
    f[flip] = f[flip][:, [0, 2, 1]]
    return f


def octahedron():
    """the regular octahedron on the unit axes -> (v float32 [6, 3], faces [8, 3], counter-clockwise seen from outside)"""
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
    f = np.array([[x, y, z] for x in (0, 1) for y in (2, 3) for z in (4, 5)], np.int64)
    return v.astype(np.float32), _outward(v, f, np.zeros(3))


def _cube(lo, side):
    v = lo + side * np.array([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)], np.float64)
    quads = [(0, 1, 3, 2), (4, 5, 7, 6), (0, 1, 5, 4), (2, 3, 7, 6), (0, 2, 6, 4), (1, 3, 7, 5)]
    f = np.array([t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))], np.int64)
    return v, _outward(v, f, lo + 0.5 * side)


def cubes():
    """two closed cubes in one mesh, [0, 1]^3 and [0.5, 1.5]^3: the winding number is 2 in [0.5, 1]^3"""
    v0, f0 = _cube(np.zeros(3), 1.0)
    v1, f1 = _cube(np.full(3, 0.5), 1.0)
    return np.concatenate([v0, v1]).astype(np.float32), np.concatenate([f0, f1 + len(v0)])


def degenerate_mesh():
    """an irregular closed octahedron, a face of zero area (three distinct collinear vertices, ids 6 .. 8) and a face over a repeated position (ids 9 and 10 hold one position)"""
    v, f = octahedron()
    v = v.astype(np.float64) * (0.9, 1.1, 0.7) + np.array([[0.05, 0.02, -0.03], [0.0, -0.04, 0.02], [0.03, 0.0, 0.05], [-0.02, 0.03, 0.0], [0.04, -0.05, 0.0], [0.0, 0.02, -0.04]])
    extra = np.array([[2, 0, 0], [2.5, 0, 0], [3, 0, 0], [0, 2, 0], [0, 2, 0], [1, 2, 0.5]], np.float64)
    return np.concatenate([v, extra]).astype(np.float32), np.concatenate([f, np.array([[6, 7, 8], [11, 9, 10]], np.int64)])


def bunny_box_cloud(count, seed, pad=0.05):
    v, _f = pref.bunny()
    lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    return np.random.default_rng(seed).uniform(lo - pad * (hi - lo), hi + pad * (hi - lo), (count, 3)).astype(np.float32)


def case(name):
    """(p, v, faces, closed) float32 / int64 of a named case; `closed`: the sign is asserted on it"""
    if name == "octahedron":
        v, f = octahedron()
        r = np.random.default_rng(61)
        return np.concatenate([r.uniform(-1.2, 1.2, (300, 3)), np.zeros((1, 3)), [[40.0, 30.0, -20.0]]]).astype(np.float32), v, f, True
    if name == "cubes":
        v, f = cubes()
        r = np.random.default_rng(62)
        return np.concatenate([r.uniform(-0.3, 1.8, (560, 3)), r.uniform(0.5, 1.0, (40, 3))]).astype(np.float32), v, f, True          # (40 points in the overlap)
    if name == "bunny":
        v, f = pref.bunny()
        return bunny_box_cloud(1500, 63), v, f, True
    if name in ("near", "regions"):
        p, v, f = pref.case(name)
        return p, v, f, True
    if name == "degenerate":                        # uniform points, the mesh's own vertices (points on a vertex) and the centroids of the two faces of zero area
        v, f = degenerate_mesh()
        r = np.random.default_rng(64)
        p = np.concatenate([r.uniform(-1.5, 3.5, (400, 3)) * (1, 1, 0.5), r.uniform(-1.0, 1.0, (200, 3)), v.astype(np.float64), v[f[-2:]].astype(np.float64).mean(1)])
        return p.astype(np.float32), v, f, True
    if name == "lattice":                           # the open mesh: no sign is asserted on it
        p, v, f = pref.sweep_reference(2049, 513)[:3]
        return p, v, f, False
    raise KeyError(name)


CASES = ("octahedron", "cubes", "bunny", "near", "regions", "degenerate")

_REF = {}


def reference(name, flipped=False):
    """a dict of a named case, computed once and shared (do not modify): p, v, f (reversed when `flipped`), closed, w64, G, w32, and the float64 and float32 nearest faces of
    tests/pointmesh_ref.py (c64, c32, computed per winding: the cascade names a face's corners in the file's order)"""
    key = (name, bool(flipped))
    if key not in _REF:
        p, v, f, closed = case(name)
        if flipped:
            f = reversed_faces(f)
        w64, G = winding(p, v, f, np.float64)
        w32, _g = winding(p, v, f, np.float32)
        if name in ("near", "regions") and not flipped:          # (pointmesh_ref's own clouds: its cache serves)
            c64, c32 = pref.reference(name)[3:]
        else:
            c64, c32 = pref.closest(p, v, f, np.float64), pref.closest(p, v, f, np.float32)
        _REF[key] = dict(p=p, v=v, f=f, closed=closed, w64=w64, G=G, w32=w32, c64=c64, c32=c32)
    return _REF[key]


def sweep_reference(max_points, max_faces):
    """the plan-boundary sweep on pointmesh_ref's lattice and cloud: (p, v, f, W64, G, W32) with W [max_points, max_faces] - column F - 1 of row i is the winding number of
    point i over the first F faces"""
    key = ("sweep", max_points, max_faces)
    if key not in _REF:
        p, v, f = pref.sweep_reference(max_points, max_faces)[:3]
        W64, G = from_matrix(theta_matrix(p, v, f, np.float64))
        W32, _g = from_matrix(theta_matrix(p, v, f, np.float32))
        _REF[key] = (p, v, f, W64, G, W32)
    return _REF[key]
