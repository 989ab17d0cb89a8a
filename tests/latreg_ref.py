"""The lattice regularisers restated in numpy from the definition in include/psdr_hip.h (THE LATTICE REGULARISERS), sharing no code with the package: plain slicing over the
lattice as an array [nz, ny, nx], in float64 - and the same statements in float32 when dtype = np.float32, which gives the error a float32 evaluation has by itself (e_32).

The sign term is here twice: sign_edges() walks the crossing edges of the seven classes and adds the two cross-entropies of each, sign_vertices() is the per-vertex form
(1 / V) sum_u m_u softplus(k |s_u|) with its gradient; tests/test_latreg_cpu.py shows them equal.

ratio() is the accuracy rule of tests/meshreg_ref.py: e_gpu <= 4 max(e_32, u G), u = 2^-24, G the largest magnitude of the float64 result, applied per
case and per term to the value and to the gradient."""
import numpy as np

U = 2.0 ** -24
CLASSES = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]          # (dx, dy, dz): the seven edge classes


def counts(shape):
    nx, ny, nz = shape
    return nx * ny * nz, (nx - 1) * (ny - 1) * (nz - 1)


def coords(shape):
    """integer coordinates [Nv, 3] of the lattice vertices, row u = x + nx (y + ny z)"""
    nx, ny, nz = shape
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], 1)


def _grid(sdf, shape, dtype):
    nx, ny, nz = shape
    return np.asarray(sdf).astype(dtype).reshape(nz, ny, nx)


def _recips(spacing, dtype):
    """1 / (4 h) and 1 / h^2, formed in float64 and rounded to dtype"""
    h = np.broadcast_to(np.asarray(spacing, np.float64), (3,))
    return [dtype(1.0 / (4.0 * a)) for a in h], [dtype(1.0 / (a * a)) for a in h]


def _lo(a, d):
    """the low ends of the edges of class d, as a view of the grid"""
    return a[: a.shape[0] - d[2], : a.shape[1] - d[1], : a.shape[2] - d[0]]


def _hi(a, d):
    return a[d[2]:, d[1]:, d[0]:]


# ---- eikonal

def cell_gradients(sdf, shape, spacing, dtype=np.float64):
    """(g_x, g_y, g_z, n) per cell [nz - 1, ny - 1, nx - 1]"""
    S = _grid(sdf, shape, dtype)
    i4, _ = _recips(spacing, dtype)
    c = lambda x, y, z: S[z: S.shape[0] - 1 + z, y: S.shape[1] - 1 + y, x: S.shape[2] - 1 + x]
    s000, s100, s010, s110, s001, s101, s011, s111 = c(0, 0, 0), c(1, 0, 0), c(0, 1, 0), c(1, 1, 0), c(0, 0, 1), c(1, 0, 1), c(0, 1, 1), c(1, 1, 1)
    gx = ((((s100 - s000) + (s110 - s010)) + (s101 - s001)) + (s111 - s011)) * i4[0]
    gy = ((((s010 - s000) + (s110 - s100)) + (s011 - s001)) + (s111 - s101)) * i4[1]
    gz = ((((s001 - s000) + (s101 - s100)) + (s011 - s010)) + (s111 - s110)) * i4[2]
    n = np.sqrt((gx * gx + gy * gy) + gz * gz)
    return gx, gy, gz, n


def eikonal(sdf, shape, spacing, dtype=np.float64):
    """-> (value, d value / d sdf [Nv])"""
    nv, nc = counts(shape)
    nx, ny, nz = shape
    i4, _ = _recips(spacing, dtype)
    gx, gy, gz, n = cell_gradients(sdf, shape, spacing, dtype)
    zero = n == 0
    safe = np.where(zero, dtype(1), n)
    d = n - dtype(1)
    e = np.where(zero, dtype(1), d * d)
    t = dtype(2) * d
    q = [np.where(zero, dtype(0), (t * (g / safe)) * i) for g, i in zip((gx, gy, gz), i4)]
    acc = [np.zeros((nz, ny, nx), dtype) for _ in range(3)]
    for b in range(8):                                             # the 8 cells around a vertex, anchors from (-1, -1, -1), x fastest
        o = ((b & 1) - 1, (b >> 1 & 1) - 1, (b >> 2 & 1) - 1)
        where = tuple(slice(1, None) if o[a] else slice(None, -1) for a in (2, 1, 0))          # the vertices that have this cell: [z, y, x]
        for a in range(3):
            if o[a]:
                acc[a][where] += q[a]                              # the vertex is the high end of axis a
            else:
                acc[a][where] -= q[a]
    grad = dtype(1.0 / nc) * ((acc[0] + acc[1]) + acc[2])
    return dtype(np.sum(e, dtype=dtype) / dtype(nc)), grad.ravel()


# ---- laplacian

def residual(sdf, shape, spacing, dtype=np.float64):
    """r_u as a grid [nz, ny, nx]"""
    S = _grid(sdf, shape, dtype)
    _, i2 = _recips(spacing, dtype)
    R = np.zeros_like(S)
    for axis, i in ((2, i2[0]), (1, i2[1]), (0, i2[2])):           # x, y, z
        if S.shape[axis] < 3:
            continue
        m = np.moveaxis(S, axis, 0)
        np.moveaxis(R, axis, 0)[1:-1] += ((m[:-2] - m[1:-1]) + (m[2:] - m[1:-1])) * i
    return R


def laplacian(sdf, shape, spacing, dtype=np.float64):
    nv, nc = counts(shape)
    _, i2 = _recips(spacing, dtype)
    R = residual(sdf, shape, spacing, dtype)
    T = []
    for axis in (2, 1, 0):
        t = np.zeros_like(R)
        if R.shape[axis] >= 3:
            r, tt = np.moveaxis(R, axis, 0), np.moveaxis(t, axis, 0)
            tt[1:-1] = dtype(-2) * r[1:-1]
            tt[2:] += r[1:-1]                                      # the neighbour one below is interior along the axis
            tt[:-2] += r[1:-1]                                     # the neighbour one above is
        T.append(t)
    grad = dtype(2.0 / nv) * ((T[0] * i2[0] + T[1] * i2[1]) + T[2] * i2[2])
    return dtype(np.sum(R * R, dtype=dtype) / dtype(nv)), grad.ravel()


# ---- sign

def inside(s):
    return s < 0


def _bce(x, y):
    return np.maximum(x, 0) - x * y + np.log1p(np.exp(-np.abs(x)))


def sign_edges(sdf, shape, k, dtype=np.float64):
    """the edge form -> (value, V)"""
    S = _grid(sdf, shape, dtype)
    k = dtype(k)
    total, V = dtype(0), 0
    for d in CLASSES:
        A, B = _lo(S, d), _hi(S, d)
        cross = inside(A) != inside(B)
        yA, yB = np.where(inside(A), dtype(0), dtype(1)), np.where(inside(B), dtype(0), dtype(1))
        both = _bce(k * A, yB) + _bce(k * B, yA)
        total = total + np.sum(both[cross], dtype=dtype)
        V += int(cross.sum())
    return (dtype(total / dtype(V)) if V else dtype(0)), V


def crossing_counts(sdf, shape):
    """m_u [nz, ny, nx]: the crossing edges among u's fourteen"""
    S = _grid(sdf, shape, np.float64)
    m = np.zeros(S.shape, np.int64)
    for d in CLASSES:
        cross = inside(_lo(S, d)) != inside(_hi(S, d))
        _lo(m, d)[...] += cross
        _hi(m, d)[...] += cross
    return m


def sign_vertices(sdf, shape, k, dtype=np.float64):
    """the per-vertex form -> (value, d value / d sdf [Nv] with V held constant, V)"""
    S = _grid(sdf, shape, dtype)
    k = dtype(k)
    m = crossing_counts(sdf, shape)
    V = int(m.sum()) // 2
    if V == 0:
        return dtype(0), np.zeros(S.size, dtype), 0
    t = k * np.abs(S)
    mf = m.astype(dtype)
    value = np.sum(mf * (t + np.log1p(np.exp(-t))), dtype=dtype) / dtype(V)
    sig = dtype(1) / (dtype(1) + np.exp(-t))
    g = (mf * sig) * (k / dtype(V))
    return dtype(value), np.where(inside(S), -g, g).ravel(), V


# ---- the loss

def reference(sdf, shape, spacing, weights=(1.0, 0.0, 0.0), sign_scale=1.0, dtype=np.float64):
    """-> {"loss", "terms" [3], "grad" [Nv], "V"}: a term of weight 0 is not evaluated and reports 0; the gradient adds the evaluated terms in the order of the weights"""
    nv, _ = counts(shape)
    terms, grad, V = [dtype(0)] * 3, None, 0
    loss = None
    for j, w in enumerate(weights):
        if not w > 0:
            continue
        if j == 0:
            value, g = eikonal(sdf, shape, spacing, dtype)
        elif j == 1:
            value, g = laplacian(sdf, shape, spacing, dtype)
        else:
            value, g, V = sign_vertices(sdf, shape, sign_scale, dtype)
        terms[j] = value
        t, tg = dtype(w) * value, dtype(w) * g
        loss, grad = (t, tg) if loss is None else (loss + t, grad + tg)
    if loss is None:
        loss, grad = dtype(0), np.zeros(nv, dtype)
    return {"loss": dtype(loss), "terms": np.array(terms, dtype), "grad": np.asarray(grad, dtype), "V": V}


def ratio(dev, f32, f64, G=None):
    """e_gpu / max(e_32, u G) (0 when everything is exactly 0), and its parts; G defaults to max |float64|"""
    dev, f32, f64 = (np.asarray(a, np.float64) for a in (dev, f32, f64))
    e_gpu, e_32 = np.abs(dev - f64).max(), np.abs(f32 - f64).max()
    G = np.abs(f64).max() if G is None else float(np.max(G))
    yard = max(e_32, U * G)
    return (0.0 if e_gpu == 0 else e_gpu / yard if yard > 0 else np.inf), e_gpu, e_32, G


# ---- the inputs

ACCURACY_SPACING = (0.1, 0.25, 0.05)
EXACT_SPACING = (0.25, 0.5, 0.125)
SIGN_SCALES = (1.0, 40.0)


def positions(shape, spacing):
    """float64 [Nv, 3]: the lattice from the origin"""
    return coords(shape) * np.asarray(spacing, np.float64)


def sphere_noise(shape, spacing, seed):
    """the distance to a sphere a little off the lattice's centre (radius: 0.3 of the longest extent), plus normal noise of a quarter of the smallest spacing"""
    P, h = positions(shape, spacing), np.asarray(spacing, np.float64)
    n = np.asarray(shape, np.float64)
    centre = 0.5 * (n - 1) * h + 0.13 * h
    radius = 0.3 * ((n - 1) * h).max()
    noise = np.random.default_rng(seed).normal(0.0, 0.25 * h.min(), len(P))
    return (np.linalg.norm(P - centre, axis=1) - radius + noise).astype(np.float32)


def pure_noise(shape, seed):
    return np.random.default_rng(seed).normal(0.0, 0.1, counts(shape)[0]).astype(np.float32)


def accuracy_shapes(tile):
    """the fixed shapes, then one below, on and one above each extent of the plan's tile and its double, then 33^3"""
    tx, ty, tz = tile
    around = lambda t: (t - 1, t, t + 1, 2 * t - 1, 2 * t, 2 * t + 1)
    fixed = [(2, 2, 2), (2, 3, 5), (5, 3, 2), (3, 3, 3), (9, 8, 7)]
    return fixed + [tuple(max(2, n) for n in s) for s in zip(around(tx), around(ty), around(tz))] + [(33, 33, 33)]


def accuracy_cases(tile):
    """[(name, shape, sdf float32 [Nv])]: two fields per shape, seeds fixed (tests/test_latreg_cpu.py asserts that none of them sits on the n = 0 kink)"""
    cases = []
    for i, shape in enumerate(accuracy_shapes(tile)):
        cases.append(("sphere+noise %s" % (shape,), shape, sphere_noise(shape, ACCURACY_SPACING, 100 + i)))
        cases.append(("noise %s" % (shape,), shape, pure_noise(shape, 200 + i)))
    return cases


def kink_margin(sdf, shape, spacing):
    """min_c n / median_c n in float64"""
    n = cell_gradients(sdf, shape, spacing)[3]
    return float(n.min() / np.median(n))
