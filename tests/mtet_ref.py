"""Marching tetrahedra in numpy: a statement of the definition of include/psdr_hip.h (THE ISOSURFACE) from its rules, for tests/test_mtet_cpu.py and tests/test_gpu_mtet.py.

Nothing here is a table over (tet, mask): the triangles of a tetrahedron come from the rules (one corner alone on its side: the slots to the other three in tet-local order;
two and two: the quad e_ik, e_il, e_jl, e_jk split along e_ik - e_jl) and every triangle's winding is found geometrically, in float64 on the unit lattice: its normal must point
from the mean of its tetrahedron's inside corners to the mean of the outside ones, or its last two slots are exchanged.  Positions and vector-Jacobian products are evaluated
in float32 with one rounding per operation, in the definition's order, and in float64.  ratio() is the rule of tests/test_gpu_meshreg.py."""
import numpy as np

U = 2.0 ** -24
PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))                  # xyz, xzy, yxz, yzx, zxy, zyx
CLASS_OFFSETS = np.array([(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)])
_CLASS_OF_CODE = np.array([-1, 0, 1, 3, 2, 4, 5, 6])                                        # dx + 2 dy + 4 dz -> class
_OTHERS = np.array([[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]])


def counts(shape):
    nx, ny, nz = shape
    return nx * ny * nz, (nx - 1) * (ny - 1) * (nz - 1)


def coords(shape, ids=None):
    """(x, y, z) of the vertex ids u = x + nx (y + ny z): int64 [n, 3]"""
    nx, ny, _nz = shape
    u = np.arange(counts(shape)[0], dtype=np.int64) if ids is None else np.asarray(ids, np.int64)
    return np.stack([u % nx, (u // nx) % ny, u // (nx * ny)], -1)


def vertex_id(shape, xyz):
    nx, ny, _nz = shape
    return xyz[..., 0] + nx * (xyz[..., 1] + ny * xyz[..., 2])


def lattice(shape, lo=-1.0, hi=1.0):
    """the regular positions float32 [Nv, 3]: lo + (hi - lo) (i / (n - 1)) in float64, rounded once"""
    lo, hi = (np.broadcast_to(np.asarray(q, np.float64), (3,)) for q in (lo, hi))
    x = coords(shape).astype(np.float64) / (np.asarray(shape, np.float64) - 1.0)
    return (lo + (hi - lo) * x).astype(np.float32)


def tets(shape):
    """the corners of every tetrahedron: int64 [6 cells, 4], row 6 cell + k = (q0, q0 + e_a, q0 + e_a + e_b, q0 + e_a + e_b + e_c) for the permutation k"""
    nx, ny, nz = shape
    c = np.arange(counts(shape)[1], dtype=np.int64)
    low = np.stack([c % (nx - 1), (c // (nx - 1)) % (ny - 1), c // ((nx - 1) * (ny - 1))], -1)
    off = np.zeros((6, 4, 3), np.int64)
    for k, perm in enumerate(PERMS):
        for step, axis in enumerate(perm):
            off[k, step + 1] = off[k, step]
            off[k, step + 1, axis] += 1
    return vertex_id(shape, low[:, None, None, :] + off[None]).reshape(-1, 4)


def inside(sdf):
    """sdf < 0: a zero is outside and so is a NaN"""
    with np.errstate(invalid="ignore"):
        return np.asarray(sdf) < 0


def edge_class(shape, a, b):
    """the class of the lattice edge from a to b = a + d_c"""
    d = coords(shape, b) - coords(shape, a)
    assert ((d == 0) | (d == 1)).all() and d.any(-1).all()
    return _CLASS_OF_CODE[d[..., 0] + 2 * d[..., 1] + 4 * d[..., 2]]


def crossing_slots(shape, ins):
    """-> (slots int64 [V] ascending, edges int32 [V, 2])"""
    X, dims = coords(shape), np.asarray(shape)
    slots, ends = [], []
    for c, d in enumerate(CLASS_OFFSETS):
        a = np.nonzero((X + d < dims).all(1))[0]
        b = vertex_id(shape, X[a] + d)
        cross = ins[a] != ins[b]
        slots.append(7 * a[cross] + c)
        ends.append(np.stack([a[cross], b[cross]], 1))
    slots, ends = np.concatenate(slots), np.concatenate(ends)
    order = np.argsort(slots, kind="stable")
    return slots[order], ends[order].astype(np.int32)


def topology(sdf, shape):
    """-> dict(edges int32 [V, 2], faces int32 [F, 3], face_tet int64 [F], slots int64 [V]): the mesh of the definition, faces in ascending tet id"""
    ins = inside(sdf)
    assert ins.shape == (counts(shape)[0],)
    slots, edges = crossing_slots(shape, ins)
    T = tets(shape)
    m = ins[T]
    n_in = m.sum(1)
    rows = np.nonzero((n_in > 0) & (n_in < 4))[0]
    T, m, n_in = T[rows], m[rows], n_in[rows]
    n = len(rows)
    pairs = np.zeros((n, 2, 3, 2), np.int64)                     # tet, triangle, slot, (local corner, local corner)
    n_tri = np.where(n_in == 2, 2, 1)
    lone = np.where(n_in == 1, m.argmax(1), (~m).argmax(1))      # the corner that is alone on its side (unused where n_in == 2)
    pairs[:, 0, :, 0] = lone[:, None]
    pairs[:, 0, :, 1] = _OTHERS[lone]
    pairs[:, 1] = pairs[:, 0]                                    # (a copy where there is no second triangle: dropped below)
    two = np.nonzero(n_in == 2)[0]
    order = np.argsort(~m[two], axis=1, kind="stable")           # inside i < j, then outside k < l
    i, j, k, l = order.T
    quad = np.stack([np.stack([i, k], 1), np.stack([i, l], 1), np.stack([j, l], 1), np.stack([j, k], 1)], 1)
    pairs[two, 0] = quad[:, [0, 1, 2]]
    pairs[two, 1] = quad[:, [0, 2, 3]]
    lo, hi = pairs.min(-1), pairs.max(-1)
    r = np.arange(n)[:, None, None]
    a, b = T[r, lo], T[r, hi]                                    # [n, 2, 3]: the anchor is the corner with the lower local index
    tri_slots = 7 * a + edge_class(shape, a, b)
    # the winding, geometrically on the unit lattice
    X = coords(shape).astype(np.float64)
    mid = (X[a] + X[b]) / 2
    normal = np.cross(mid[:, :, 1] - mid[:, :, 0], mid[:, :, 2] - mid[:, :, 0])
    corners = X[T]
    w_in = m[:, :, None].astype(np.float64)
    direction = ((1 - w_in) * corners).sum(1) / (4 - n_in)[:, None] - (w_in * corners).sum(1) / n_in[:, None]
    side = (normal * direction[:, None, :]).sum(-1)              # [n, 2]
    valid = np.arange(2)[None, :] < n_tri[:, None]
    assert (side[valid] != 0).all()
    swap = side < 0
    tri_slots[swap] = tri_slots[swap][:, [0, 2, 1]]
    flat = tri_slots[valid]                                      # row-major: ascending tet, then the triangle's number
    index = np.searchsorted(slots, flat)
    assert (index < max(len(slots), 1)).all() and (len(flat) == 0 or (slots[index] == flat).all()), "a face names a slot that does not cross"
    face_tet = np.broadcast_to(rows[:, None], (n, 2))[valid]
    return {"edges": edges, "faces": index.astype(np.int32).reshape(-1, 3), "face_tet": face_tet, "slots": slots}


def canonical(faces):
    """faces as a set: every triangle rotated so that its smallest vertex index comes first, the rows sorted"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    k = f.argmin(1)
    f = f[np.arange(len(f))[:, None], (k[:, None] + np.arange(3)) % 3]
    return f[np.lexsort((f[:, 2], f[:, 1], f[:, 0]))]


def positions(sdf, pos, edges, dtype=np.float64):
    """p = p_a + t (p_b - p_a), t = s_a / (s_a - s_b): one rounding of `dtype` per operation"""
    s, p = np.asarray(sdf).astype(dtype), np.asarray(pos).astype(dtype)
    a, b = np.asarray(edges)[:, 0], np.asarray(edges)[:, 1]
    with np.errstate(all="ignore"):
        t = s[a] / (s[a] - s[b])
        return p[a] + t[:, None] * (p[b] - p[a])


def vjp(sdf, pos, edges, g, shape, dtype=np.float64):
    """(g . dv / dsdf [Nv], g . dv / dpos [Nv, 3]) with the topology held constant, in the definition's order: a lattice vertex adds, from 0, its own slots in ascending class
    and then the slots it is the far end of in ascending class"""
    s, p, g = np.asarray(sdf).astype(dtype), np.asarray(pos).astype(dtype), np.asarray(g).astype(dtype)
    a, b = np.asarray(edges)[:, 0].astype(np.int64), np.asarray(edges)[:, 1].astype(np.int64)
    cls = edge_class(shape, a, b)
    with np.errstate(all="ignore"):
        d, den = p[b] - p[a], s[a] - s[b]
        t = s[a] / den
        w = ((g[:, 0] * d[:, 0] + g[:, 1] * d[:, 1]) + g[:, 2] * d[:, 2]) / (den * den)
        ds_a, ds_b = (-s[b]) * w, s[a] * w
        dp_a, dp_b = (dtype(1) - t)[:, None] * g, t[:, None] * g
        gs, gp = np.zeros(len(s), dtype), np.zeros((len(s), 3), dtype)
        for end, ds, dp in ((a, ds_a, dp_a), (b, ds_b, dp_b)):
            for c in range(7):
                sel = cls == c                                   # (a lattice vertex has at most one slot of a class at either end: the indices are unique)
                gs[end[sel]] = gs[end[sel]] + ds[sel]
                gp[end[sel]] = gp[end[sel]] + dp[sel]
    return gs, gp


def ratio(dev, f32, f64):
    """e_gpu / max(e_32, u G) (0 when everything is exactly 0), and its parts; G = max |float64|"""
    dev, f32, f64 = (np.asarray(x, np.float64) for x in (dev, f32, f64))
    if dev.size == 0:
        return 0.0, 0.0, 0.0, 0.0
    e_gpu, e_32, G = np.abs(dev - f64).max(), np.abs(f32 - f64).max(), np.abs(f64).max()
    yard = max(e_32, U * G)
    return (0.0 if e_gpu == 0 else e_gpu / yard if yard > 0 else np.inf), e_gpu, e_32, G


# ---- the mesh as a surface

def directed_edge_counts(faces):
    """{(i, j): the number of triangles that run from i to j}"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    uniq, n = np.unique(e, axis=0, return_counts=True)
    return {(int(i), int(j)): int(k) for (i, j), k in zip(uniq, n)}


def closed_and_oriented(faces):
    """every directed edge is used once and so is its reverse"""
    dc = directed_edge_counts(faces)
    return len(dc) > 0 and all(k == 1 and dc.get((j, i)) == 1 for (i, j), k in dc.items())


def euler(faces, n_vertices):
    dc = directed_edge_counts(faces)
    return n_vertices - len({(min(e), max(e)) for e in dc}) + len(np.asarray(faces).reshape(-1, 3))


def signed_volume(v, faces):
    v, f = np.asarray(v, np.float64), np.asarray(faces, np.int64).reshape(-1, 3)
    return float((v[f[:, 0]] * np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)


# ---- the inputs

SPHERE_SHAPE, SPHERE_CENTRE, SPHERE_RADIUS = (12, 11, 10), np.array([0.031, -0.047, 0.052]), 0.642          # no lattice vertex within 3e-3 of the surface (asserted by the tests)


def sphere(shape=SPHERE_SHAPE, centre=SPHERE_CENTRE, radius=SPHERE_RADIUS):
    """-> (pos float32 [Nv, 3] on [-1, 1]^3, sdf float32 [Nv]): the distance to a sphere, evaluated in float64 at the float32 positions"""
    pos = lattice(shape, -1.0, 1.0)
    sdf = (np.linalg.norm(pos.astype(np.float64) - centre, axis=1) - radius).astype(np.float32)
    return pos, sdf


def cell_diagonal(shape, lo=-1.0, hi=1.0):
    return float(np.linalg.norm((hi - lo) / (np.asarray(shape, np.float64) - 1.0)))


def jittered(shape, seed, amount=0.2):
    """a deformed lattice: the regular one on [0, n - 1]^3 moved by at most `amount` of a cell per axis"""
    r = np.random.default_rng(seed)
    return (coords(shape).astype(np.float64) + r.uniform(-amount, amount, (counts(shape)[0], 3))).astype(np.float32)


def random_sdf(shape, seed, keep_away=0.0):
    """normally distributed values, pushed away from zero by `keep_away`"""
    s = np.random.default_rng(seed).standard_normal(counts(shape)[0])
    return (s + np.sign(s) * keep_away).astype(np.float32)


_CACHE = {}


def reference(sdf, pos, shape, g=None, key=None):
    """the topology of (sdf, shape) and, with pos, the positions in float32 / float64 and, with g [V, 3], both vector-Jacobian products in both precisions; computed once
    per key and left unchanged"""
    if key is not None and key in _CACHE:
        return _CACHE[key]
    r = topology(sdf, shape)
    if pos is not None:
        r["v32"], r["v64"] = positions(sdf, pos, r["edges"], np.float32), positions(sdf, pos, r["edges"], np.float64)
    if g is not None:
        r["gs32"], r["gp32"] = vjp(sdf, pos, r["edges"], g, shape, np.float32)
        r["gs64"], r["gp64"] = vjp(sdf, pos, r["edges"], g, shape, np.float64)
    if key is not None:
        _CACHE[key] = r
    return r
