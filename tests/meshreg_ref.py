"""An independent reading of the mesh regularisers (include/psdr_hip.h states the definition; psdr_jit_amd/meshreg.py and csrc/hip/meshreg.hip implement it): shares no code
with the package.  topology() is a per-face Python loop over dictionaries; evaluate() gives the three values and their gradients from analytic per-element gradients summed
per vertex, in float64 numpy - or, with dtype=np.float32, the same statements in float32 with numpy's own summation order (pairwise np.sum for the values, np.add.at in
element order for the per-vertex sums).  That float32 evaluation is the yardstick of the accuracy rule:

    e_gpu = max |device - float64|,  e_32 = max |float32 checker - float64|,  G = max |float64|,  u = 2^-24:      e_gpu <= 4 max(e_32, u G)

per case, per term, for the value and for the gradient (ratio() returns e_gpu / max(e_32, u G)).  The factor 4 covers another summation order and the device's division and
square root; the floor u G is one rounding of the largest entry and keeps a nine-entry case from being judged against a lucky e_32.  Accuracy cases use vertices in general
position (case()): unit-spaced grids with a normal jitter of sigma = 0.01, the bunny scaled into the unit cube, uniform positions in [-1, 1]^3 otherwise, all rounded
to float32.  Meshes come from tests/subdiv_ref.py."""
import numpy as np

import subdiv_ref as sref

U = 2.0 ** -24
TINY = 2.0 ** -100


def topology(faces, n):
    """dict: edges [(a, b)] sorted, hinges [(a, b, c, d)] in edge order, boundary / nonmanifold counts, neighbours [sorted list per vertex], and the inverted indices
    edge_index / hinge_index [list of (element, role) per vertex, ascending]"""
    at = {}                                          # undirected edge -> [(face index, the face's third vertex)]
    for k, (a, b, c) in enumerate(faces):
        for p, q, o in ((a, b, c), (b, c, a), (c, a, b)):
            at.setdefault((min(p, q), max(p, q)), []).append((k, o))
    edges = sorted(at)
    hinges, boundary, nonmanifold = [], 0, 0
    for e in edges:
        inc = sorted(at[e])
        if len(inc) == 2:
            hinges.append((e[0], e[1], inc[0][1], inc[1][1]))
        elif len(inc) == 1:
            boundary += 1
        else:
            nonmanifold += 1
    neighbours = [set() for _ in range(n)]
    for a, b in edges:
        neighbours[a].add(b)
        neighbours[b].add(a)
    edge_index, hinge_index = [[] for _ in range(n)], [[] for _ in range(n)]
    for k, e in enumerate(edges):
        for role, v in enumerate(e):
            edge_index[v].append((k, role))
    for k, hg in enumerate(hinges):
        for role, v in enumerate(hg):
            hinge_index[v].append((k, role))
    return {"edges": edges, "hinges": hinges, "boundary": boundary, "nonmanifold": nonmanifold, "neighbours": [sorted(s) for s in neighbours],
            "edge_index": edge_index, "hinge_index": hinge_index}


def _dot(a, b):
    return (a * b).sum(1)


def evaluate(V, faces, n, target_length=0.0, dtype=np.float64, topo=None):
    """-> {"laplacian", "normal", "edge": (value, gradient [n, 3])}, unweighted, every operation in `dtype`"""
    t = topology(faces, n) if topo is None else topo
    T = dtype
    V = np.asarray(V).astype(T)
    assert V.shape == (n, 3)
    out = {}
    # laplacian
    pairs = np.array([(i, j) for i in range(n) for j in t["neighbours"][i]], dtype=np.int64).reshape(-1, 2)
    deg = np.array([len(s) for s in t["neighbours"]], dtype=np.int64)
    used = deg > 0
    n_l = int(used.sum())
    s = np.zeros((n, 3), T)
    np.add.at(s, pairs[:, 0], V[pairs[:, 1]])
    degT = np.maximum(deg, 1).astype(T)[:, None]
    delta = np.where(used[:, None], V - s / degT, T(0))
    if n_l:
        q = delta / degT
        back = np.zeros((n, 3), T)
        np.add.at(back, pairs[:, 0], q[pairs[:, 1]])
        out["laplacian"] = (T(_dot(delta, delta).sum() / T(n_l)), (T(2) / T(n_l)) * (delta - back))
    else:
        out["laplacian"] = (T(0), np.zeros((n, 3), T))
    # normal
    H = np.array(t["hinges"], dtype=np.int64).reshape(-1, 4)
    g = np.zeros((n, 3), T)
    if len(H):
        a, b, c, d = (V[H[:, k]] for k in range(4))
        e0, p, q = b - a, c - a, d - a
        n1, n2 = np.cross(e0, p), np.cross(q, e0)
        l1, l2 = _dot(n1, n1), _dot(n2, n2)
        ok = ~((l1 < T(TINY)) | (l2 < T(TINY)))
        r1, r2 = np.sqrt(np.where(ok, l1, T(1)))[:, None], np.sqrt(np.where(ok, l2, T(1)))[:, None]
        u1, u2 = n1 / r1, n2 / r2
        w = u1 - u2
        val = np.where(ok, T(0.5) * _dot(w, w), T(0))
        g1 = (w - _dot(u1, w)[:, None] * u1) / r1             # d / dn1
        g2 = -(w - _dot(u2, w)[:, None] * u2) / r2            # d / dn2
        gb = np.cross(p, g1) + np.cross(g2, q)
        gc = np.cross(g1, e0)
        gd = np.cross(e0, g2)
        ga = -(gb + gc + gd)
        for k, gk in enumerate((ga, gb, gc, gd)):
            np.add.at(g, H[:, k], np.where(ok[:, None], gk, T(0)))
        out["normal"] = (T(val.sum() / T(len(H))), g / T(len(H)))
    else:
        out["normal"] = (T(0), g)
    # edge
    E = np.array(t["edges"], dtype=np.int64).reshape(-1, 2)
    g = np.zeros((n, 3), T)
    if len(E):
        L0 = T(target_length)
        d = V[E[:, 0]] - V[E[:, 1]]
        l2 = _dot(d, d)
        if L0 == 0:
            val, ge = l2, T(2) * d
        else:
            ok = ~(l2 < T(TINY))
            l = np.sqrt(np.where(ok, l2, T(1)))
            r = l - L0
            val = np.where(ok, r * r, L0 * L0)
            ge = np.where(ok[:, None], (T(2) * r / l)[:, None] * d, T(0))
        np.add.at(g, E[:, 0], ge)
        np.add.at(g, E[:, 1], -ge)
        out["edge"] = (T(val.sum() / T(len(E))), g / T(len(E)))
    else:
        out["edge"] = (T(0), g)
    return out


TERMS = ("laplacian", "normal", "edge")


def combine(res, weights, dtype=np.float64):
    """(loss, gradient) = the weighted sum of the terms in the definition's order, terms of weight 0 left out"""
    loss, grad = dtype(0), None
    for name, w in zip(TERMS, weights):
        if w > 0:
            loss = loss + dtype(w) * res[name][0]
            grad = dtype(w) * res[name][1] if grad is None else grad + dtype(w) * res[name][1]
    if grad is None:
        grad = np.zeros_like(res["edge"][1])
    return dtype(loss), grad


def ratio(dev, f32, f64):
    """e_gpu / max(e_32, u G) (0 when everything is exactly 0), and its parts"""
    dev, f32, f64 = (np.asarray(x, np.float64) for x in (dev, f32, f64))
    e_gpu, e_32, G = np.abs(dev - f64).max(), np.abs(f32 - f64).max(), np.abs(f64).max()
    yard = max(e_32, U * G)
    return (0.0 if e_gpu == 0 else e_gpu / yard if yard > 0 else np.inf), e_gpu, e_32, G


# ---- the meshes and their positions in general position

def _uniform(n, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (n, 3)).astype(np.float32)


def _grid_positions(m, seed):
    ij = np.stack(np.meshgrid(np.arange(m), np.arange(m), indexing="ij"), -1).reshape(-1, 2).astype(np.float64)
    z = np.random.default_rng(seed).normal(0.0, 0.01, m * m)
    return np.concatenate([ij, z[:, None]], 1).astype(np.float32)


_BUNNY = []


def bunny():
    """(faces, n, positions scaled into the unit cube, float32)"""
    if not _BUNNY:
        f, n, v, _ft, _vt = sref.load_obj(sref.BUNNY)
        v = (v - v.min(0)) / (v.max(0) - v.min(0)).max()
        _BUNNY.append((f, n, v.astype(np.float32)))
    return _BUNNY[0]


def case(name):
    """(faces, n, positions float32 [n, 3]) of a named accuracy case"""
    if name == "point":
        return [], 1, _uniform(1, 1)
    if name == "triangle":
        return [[0, 1, 2]], 3, _uniform(3, 2)
    if name == "fold":
        return [[0, 1, 2], [1, 0, 3]], 4, _uniform(4, 3)
    if name == "tetrahedron":
        return sref.TETRAHEDRON, 4, _uniform(4, 4)
    if name == "bowtie":
        return sref.BOWTIE, 5, _uniform(5, 5)
    if name == "book":
        return sref.BOOK, 5, _uniform(5, 6)
    if name.startswith("fan"):
        f, n = sref.fan(int(name[3:]))
        return f, n, _uniform(n, 7)
    if name.startswith("grid"):
        m = int(name[4:])
        f, n = sref.grid(m)
        return f, n, _grid_positions(m, 8)
    if name == "bunny":
        return bunny()
    if name == "degenerate":
        return degenerate()
    raise KeyError(name)


def degenerate():
    """(faces, n, positions float32): face (1, 2, 4) has zero area (vertex 4 is the exact midpoint of the edge 1 - 2, whose ends are multiples of 2^-10) and so has face
    (2, 0, 5), where vertex 5 sits on vertex 2: the edge (2, 5) has zero length.  The hinges (1, 2, 0, 4) and (0, 2, 1, 5) have a zero normal in every arithmetic."""
    v = _uniform(6, 11)
    v[1:3] = np.round(v[1:3] * 1024.0) / 1024.0
    v[4] = 0.5 * (v[1] + v[2])
    v[5] = v[2]
    return [[0, 1, 2], [1, 0, 3], [1, 2, 4], [2, 0, 5]], 6, v


CASES = ("point", "triangle", "fold", "tetrahedron", "bowtie", "book", "fan5", "fan70", "grid3", "grid17", "grid27", "bunny")

_REF = {}


def reference(name, target_length):
    """(float64 result, float32 result, topology) of a named case, computed once and shared (do not modify)"""
    key = (name, float(target_length))
    if key not in _REF:
        f, n, v = case(name)
        t = _REF[(name, "topo")] if (name, "topo") in _REF else _REF.setdefault((name, "topo"), topology(f, n))
        _REF[key] = (evaluate(v, f, n, target_length, np.float64, t), evaluate(v, f, n, target_length, np.float32, t), t)
    return _REF[key]
