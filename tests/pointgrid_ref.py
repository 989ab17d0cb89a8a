"""A numpy restatement of the grid search (include/psdr_hip.h states the contract; csrc/hip/nn_grid.h implements it): the cell function, the build, the shell walk with
its stopping rule and the fallback, every float operation a numpy float32 operation in the kernel's order.  It shares no code with the package; the plan (res,
max_shells) is passed in.  It is the CPU proof of the stopping rule - test_pointgrid_cpu.py compares it with chamfer_ref.nearest bit for bit - and it counts what the
device counts: the queries the fallback finishes and the (query, candidate) pairs tested.

The pairs are well defined by the contract's schedule-free part: a query tests every candidate of every cell of every shell it visits (shells 0 .. s*, s* the first
shell after which it is certified, or max_shells - 1), and all m candidates once more if the fallback takes it.  The device's walk tests exactly those, whatever the lanes that share a query.

check_build holds a built PointGrid to the restatement's Grid array by array.  The named cases (case, CASES) put the search on each of its paths: res 8 - 11 for the
first fifteen, shell budgets 4 to 16 for the cavity cases, awkward float32 coordinates and symmetric or hollow clouds for the geometry cases; scan_pass gives the sizes at
which the build's exclusive scan changes its number of chunks."""
import numpy as np

import chamfer_ref as cref

F = np.float32
WALK = 8          # steps that the search for a plane may take, the first 2^-22 max(|lo|, |hi|) long and each twice the one before (nn_grid.h: kWalk)


def cell_of(v, lo, inv, dim):
    """c(v) = clamp(floor((v - lo) * inv), 0, dim - 1) in float32, a NaN to cell 0; v an array or a scalar"""
    with np.errstate(all="ignore"):
        t = np.floor((np.asarray(v, F) - F(lo)) * F(inv))
        t = np.where(t >= 0, t, F(0))
        t = np.minimum(t, F(dim - 1))
    return t.astype(np.int64)


def axis_constants(lo, hi, res):
    """(inv, width, dim) of an axis whose candidates span [lo, hi]: an axis of zero extent, or an inv that is not finite and positive, has one cell"""
    with np.errstate(all="ignore"):
        extent = F(hi) - F(lo)
        inv = F(res) / extent
        width = extent / F(res)
    many = bool(inv > 0 and inv < np.inf)
    return F(inv), F(width), (res if many else 1)


def plane(lo, hi, inv, width, dim, side, k):
    """side 0, 1 <= k < dim: a float b with c(b) < k (else -inf); side 1, 0 <= k < dim - 1: a float b with c(b) > k (else +inf)"""
    lo, inv, width = F(lo), F(inv), F(width)
    with np.errstate(all="ignore"):
        return _plane(lo, np.maximum(np.abs(lo), np.abs(F(hi))) * F(2.0 ** -22), inv, width, dim, side, k)


def _plane(lo, d, inv, width, dim, side, k):
    if side == 0:
        if not 1 <= k < dim:
            return F(-np.inf)
        b = lo + F(k) * width
        for _ in range(WALK + 1):
            if cell_of(b, lo, inv, dim) < k:
                return F(b)
            b, d = F(b - d), F(d + d)
        return F(-np.inf)
    if not 0 <= k < dim - 1:
        return F(np.inf)
    b = lo + F(k + 1) * width
    for _ in range(WALK + 1):
        if cell_of(b, lo, inv, dim) > k:
            return F(b)
        b, d = F(b + d), F(d + d)
    return F(np.inf)


class Grid:
    """the build: box, constants, planes, cell_begin [res^3 + 1] and the candidates in cell order (stable, which the device's need not be: nothing depends on it)"""

    def __init__(self, y, res):
        y = np.ascontiguousarray(y, F)
        self.y, self.m, self.res = y, len(y), int(res)
        self.lo = y.min(0) + F(0)
        self.hi = hi = y.max(0) + F(0)
        consts = [axis_constants(self.lo[a], hi[a], res) for a in range(3)]
        self.inv = np.array([c[0] for c in consts], F)
        self.width = np.array([c[1] for c in consts], F)
        self.dim = [c[2] for c in consts]
        self.up = np.array([[plane(self.lo[a], self.hi[a], self.inv[a], self.width[a], self.dim[a], 0, k) for k in range(res)] for a in range(3)], F)
        self.down = np.array([[plane(self.lo[a], self.hi[a], self.inv[a], self.width[a], self.dim[a], 1, k) for k in range(res)] for a in range(3)], F)
        c = self.cells_of(y)
        cell = (c[:, 0] * res + c[:, 1]) * res + c[:, 2]
        self.order = np.argsort(cell, kind="stable")
        self.begin = np.zeros(res ** 3 + 1, np.int64)
        np.cumsum(np.bincount(cell, minlength=res ** 3), out=self.begin[1:])
        self.sorted = y[self.order]

    def cells_of(self, p):
        return np.stack([cell_of(p[:, a], self.lo[a], self.inv[a], self.dim[a]) for a in range(3)], 1)


def _test_ranges(x, G, b0, b1, best, bj):
    """every query q (rows of x) against the sorted candidates [b0[q], b1[q]): the lexicographic minimum over (d2, j), merged into (best, bj) in place"""
    length = b1 - b0
    for t in range(int(length.max()) if len(length) else 0):
        on = np.nonzero(length > t)[0]
        at = b0[on] + t
        p, j = G.sorted[at], G.order[at]
        q = x[on]
        dx, dy, dz = q[:, 0] - p[:, 0], q[:, 1] - p[:, 1], q[:, 2] - p[:, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        assert d2.dtype == F
        win = (d2 < best[on]) | ((d2 == best[on]) & (j < bj[on]))
        best[on[win]], bj[on[win]] = d2[win], j[win]


def nearest(x, y, res, max_shells):
    """-> (index int32 [N], dist2 float32 [N], stats): stats = {"fallback": queries the fallback finished, "pairs": pairs tested in all, "walk_pairs": by the shell walk
    alone, "shells": per query the shells visited, "walk_pairs_of": per query the pairs its walk tested, "fell": per query whether the fallback took it, "grid": the Grid}"""
    x = np.ascontiguousarray(x, F)
    G = Grid(y, res)
    n, m = len(x), G.m
    c = G.cells_of(x)
    best, bj = np.full(n, np.inf, F), np.zeros(n, np.int64)
    live = np.arange(n)                                  # the queries not yet certified
    shells = np.zeros(n, np.int64)
    walk_pairs_of = np.zeros(n, np.int64)
    with np.errstate(all="ignore"):
        for s in range(max_shells):
            if not len(live):
                break
            cl, xl = c[live], x[live]
            bl, jl = best[live], bj[live]
            shells[live] += 1
            for d0 in range(-s, s + 1):
                for d1 in range(-s, s + 1):
                    c0, c1 = cl[:, 0] + d0, cl[:, 1] + d1
                    inside = (c0 >= 0) & (c0 < G.dim[0]) & (c1 >= 0) & (c1 < G.dim[1])
                    rim = max(abs(d0), abs(d1)) == s
                    runs = [(np.maximum(cl[:, 2] - s, 0), np.minimum(cl[:, 2] + s, G.dim[2] - 1))] if rim else [(cl[:, 2] - s, cl[:, 2] - s), (cl[:, 2] + s, cl[:, 2] + s)]
                    for z0, z1 in runs:
                        ok = inside & (z0 >= 0) & (z1 < G.dim[2]) & (z0 <= z1)
                        row = (np.where(ok, c0, 0) * res + np.where(ok, c1, 0)) * res
                        b0 = np.where(ok, G.begin[row + np.where(ok, z0, 0)], 0)
                        b1 = np.where(ok, G.begin[row + np.where(ok, z1, 0) + 1], 0)
                        walk_pairs_of[live] += b1 - b0
                        _test_ranges(xl, G, b0, b1, bl, jl)
            best[live], bj[live] = bl, jl
            done = np.ones(len(live), bool)
            for a in range(3):
                up, down = cl[:, a] + s + 1, cl[:, a] - s - 1
                has = up < G.dim[a]
                gap = G.up[a][np.where(has, up, 0)] - xl[:, a]
                done &= ~has | ((gap >= 0) & (gap * gap > bl))
                has = down >= 0
                gap = xl[:, a] - G.down[a][np.where(has, down, 0)]
                done &= ~has | ((gap >= 0) & (gap * gap > bl))
            live = live[~done]
    if len(live):                                         # the fallback: the definition's scan over all m candidates
        fi, fd = cref.nearest(x[live], G.y)
        bj[live], best[live] = fi, fd
    fell = np.zeros(n, bool)
    fell[live] = True
    walk_pairs = int(walk_pairs_of.sum())
    stats = {"fallback": int(len(live)), "walk_pairs": walk_pairs, "pairs": walk_pairs + int(len(live)) * m, "shells": shells, "walk_pairs_of": walk_pairs_of, "fell": fell, "grid": G}
    return bj.astype(np.int32), best, stats


def _host(t):
    return np.ascontiguousarray(t.cpu().numpy() if hasattr(t, "cpu") else t)


def _first(a, b, what):
    """a and b are equal entry for entry (floats by their bits), or the first difference is named"""
    a, b = _host(a).ravel(), _host(b).ravel()
    assert a.shape == b.shape, "%s: %d entries, expected %d" % (what, a.size, b.size)
    if a.dtype == F:
        assert b.dtype == F
        a, b = a.view(np.uint32), b.view(np.uint32)
    bad = np.nonzero(a != b)[0]
    assert bad.size == 0, "%s: %d of %d entries differ, first at %d: %r, expected %r" % (what, bad.size, a.size, bad[0], a[bad[0]], b[bad[0]])


def check_build(grid, G, what=""):
    """A built grid (a PointGrid of the package: box, dims, planes, cell_begin, sorted, points; device tensors or numpy arrays) against the restatement's Grid of the
    same candidates, array by array and without a tolerance: the box constants and every plane by their bits, infinities included, every entry of cell_begin, and the
    sorted candidates as far as they are defined - the index column a permutation of 0 .. m - 1, row t the point of its index bit for bit, and inside every cell the
    same set of indices as the restatement's (the order inside a cell is not defined)."""
    res, m = G.res, G.m
    _first(grid.points, G.y, what + " points")
    _first(grid.box, np.concatenate([G.lo, G.inv, G.width]).astype(F), what + " box (lo, inv, width)")
    _first(_host(grid.dims).astype(np.int64), np.array(G.dim, np.int64), what + " dims")
    planes = np.stack([np.stack([G.up[a], G.down[a]]) for a in range(3)]).astype(F)          # plane (axis a, side, k) at (2 a + side) res + k
    assert planes.shape == (3, 2, res)
    _first(grid.planes, planes, what + " planes")
    _first(_host(grid.cell_begin).astype(np.int64), G.begin, what + " cell_begin")
    rows = _host(grid.sorted).view(np.int32).reshape(-1, 4)
    assert rows.shape == (m, 4), what
    index = rows[:, 3].astype(np.int64)
    _first(np.sort(index), np.arange(m), what + " sorted: the index column is no permutation")
    _first(rows[:, :3], G.y.view(np.int32)[index], what + " sorted: a row is not the point of its index")
    cell = np.repeat(np.arange(res ** 3, dtype=np.int64), np.diff(G.begin))                    # the cell of every slot of the sorted order
    _first(np.sort(cell * m + index), cell * m + G.order, what + " sorted: the indices of a cell")      # (G.order is ascending inside a cell: the sort was stable)


# ---- the named cases: (x, y) float32; `plan` is the package's grid_plan and sizes are read from it

def res_changes(plan, top=8):
    """the m at which res changes, from res 1 up to `top`: [m_2, m_3, ...], m_r the smallest m with res == r (bisection; res is monotone in m)"""
    out = []
    for r in range(2, top + 1):
        lo, hi = 1, 1 << 26
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if plan(1, mid).res >= r else (mid, hi)
        out.append(hi)
    return out


def _uniform(n, seed, lo=-1.0, hi=1.0):
    return np.random.default_rng(seed).uniform(lo, hi, (n, 3)).astype(F)


def _m_for_res(plan, r):
    """the smallest m with res == r (one bisection; res is monotone in m)"""
    lo, hi = 0, 1 << 26
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if plan(1, mid).res >= r else (mid, hi)
    return hi


def scan_chunks(plan, m, work_head):
    """the workgroups of the build's exclusive scan over the cells (2048 cells each), read from the plan: what work_words holds beyond its head (the package's
    WORK_HEAD) and the two per-candidate arrays.  k_grid_scan_top gives each of its 1024 lanes ceil(chunks / 1024) of them: more than one from 1025 chunks on"""
    return plan(1, m).work_words - work_head - 2 * m


def _unit(r, n):
    d = r.normal(size=(n, 3))
    return d / np.sqrt((d * d).sum(1))[:, None]


CAVITY_BUDGETS = (4, 5, 8, 12, 16)
CAVITY_RADIUS = 0.75


def case(name, plan):
    m8 = _m_for_res(plan, 8)                     # the smallest m with res = 8
    r = np.random.default_rng(sum(map(ord, name)))
    if name == "uniform":                       # a full box, more than one workgroup of queries
        return _uniform(1500, 1), _uniform(m8 + 321, 2)
    if name == "lattice":                       # an 8^3 lattice in multiples of 2^-6; the queries on the lattice and on cell faces (half steps): exact ties across cells
        y = (np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), -1).reshape(-1, 3) / 64.0).astype(F)
        y = np.concatenate([y, y[r.integers(0, 512, m8)]])[r.permutation(512 + m8)]
        x = (r.integers(0, 15, (900, 3)) / 128.0).astype(F)
        return x, np.ascontiguousarray(y)
    if name in ("tie_far_low", "tie_near_low"):  # two candidates at exactly the same distance from every query, one in the query's cell, one a shell farther out; the
        y = _uniform(m8, 3, 2.0, 3.0)            # lower index is the far one (tie_far_low) or the near one
        y[0], y[1] = (0.0, 0.0, 0.0), (3.0, 3.0, 3.0)          # the box's corners: res = 8 gives cells of width 3 / 8
        x = np.array([[0.4375, 0.125, 0.125]], F).repeat(70, 0)                    # cell 1 along axis 0
        near, far = np.array([0.6875, 0.125, 0.125], F), np.array([0.1875, 0.125, 0.125], F)          # both at 0.25 exactly: cell 1 (shell 0) and cell 0 (shell 1)
        y[5], y[m8 - 3] = (far, near) if name == "tie_far_low" else (near, far)
        return x, y
    if name == "copies":                        # exact copies of the winner in the same cell, a neighbouring cell's worth away and far away in index order
        y = _uniform(m8 + 100, 4)
        x = (y[::7] + F(1e-3) * _uniform(len(y[::7]), 5)).astype(F)
        extra = np.concatenate([y[::7], y[::7]])
        y = np.concatenate([y, extra])
        return x, y
    if name == "identical_y":
        return _uniform(300, 7), np.repeat(_uniform(1, 8), m8 + 3, 0)
    if name == "same":
        x = _uniform(m8 + 300, 9)
        return x, x.copy()
    if name == "planar":                        # one axis of zero extent
        y = _uniform(m8 + 50, 10)
        y[:, 1] = F(0.25)
        x = _uniform(700, 11)
        x[:, 1] = (F(0.25) + F(0.05) * x[:, 1]).astype(F)
        return x, y
    if name == "collinear":                     # two axes of zero extent
        y = _uniform(m8 + 50, 12)
        y[:, 0], y[:, 2] = F(-0.5), F(3.0)
        x = _uniform(700, 13)
        x[:, 0], x[:, 2] = (F(-0.5) + F(0.002) * x[:, 0]).astype(F), (F(3.0) + F(0.002) * x[:, 2]).astype(F)
        return x, y
    if name == "far":                           # coordinates around 1000 with a spacing of 1e-3
        x = (1000.0 + 1e-3 * r.integers(-40, 40, (500, 3)) + 2e-4 * r.uniform(-1, 1, (500, 3))).astype(F)
        y = (1000.0 + 1e-3 * r.integers(-40, 40, (3 * m8 - 7, 3)) + 2e-4 * r.uniform(-1, 1, (3 * m8 - 7, 3))).astype(F)
        return x, y
    if name == "outside_near":                  # queries one cell outside the box, on every side
        y = _uniform(m8 + 77, 14)
        w = 2.0 / plan(1, len(y)).res
        x = _uniform(600, 15)
        side = r.integers(0, 6, 600)
        for a in range(3):
            x[side == 2 * a, a] = F(-1.0 - w) + F(0.5 * w) * x[side == 2 * a, a]
            x[side == 2 * a + 1, a] = F(1.0 + w) + F(0.5 * w) * x[side == 2 * a + 1, a]
        return x, y
    if name == "outside_far":                   # queries 100 extents away
        y = _uniform(m8 + 77, 16)
        x = (_uniform(300, 17) + np.array([200.0, -200.0, 200.0], F) * r.choice([-1.0, 1.0], (300, 3)).astype(F)).astype(F)
        return x, y
    if name == "clusters":                      # two clusters a hundred cluster-widths apart, the queries between them
        a, b = _uniform(m8 // 2 + 5, 18, 0.0, 1.0), _uniform(m8 // 2 + 6, 19, 0.0, 1.0) + np.array([100.0, 0.0, 0.0], F)
        y = np.concatenate([a, b.astype(F)])[r.permutation(m8 + 11)]
        x = _uniform(400, 20, 0.0, 1.0)
        x[:, 0] = (F(1.5) + F(97.0) * x[:, 0]).astype(F)
        return x, np.ascontiguousarray(y)
    if name == "hub":                           # one cell holds all but ten candidates
        y = (F(0.5) + F(1e-3) * _uniform(m8 + 40, 21)).astype(F)
        y[:10] = _uniform(10, 22)
        y[0], y[1] = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
        return _uniform(300, 23), y
    if name == "bunny":                         # the bunny's vertices against a jittered copy
        v, _f = cref.bunny()
        return v, (v + np.random.default_rng(12).normal(0.0, 0.01, v.shape)).astype(F)
    if name.startswith("cavity_"):              # a full box with a ball cut out of it, the queries in the hollow at every depth: every shell count up to the budget k
        k = int(name[len("cavity_"):])          # occurs and the deepest queries fall back.  m is the smallest m with max_shells == k: res = 4 k, m = 2 res^3
        m = _m_for_res(plan, 4 * k)
        assert plan(1, m).res == 4 * k and plan(1, m).max_shells == k
        parts, have = [], 0
        while have < m:                         # (rejection from the one generator until m remain)
            c = r.uniform(-1.0, 1.0, (m, 3)).astype(F)
            c = c[(c.astype(np.float64) ** 2).sum(1) >= CAVITY_RADIUS ** 2]
            parts.append(c)
            have += len(c)
        y = np.ascontiguousarray(np.concatenate(parts)[:m])
        y[0], y[1] = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
        depth = np.linspace(0.0, CAVITY_RADIUS, 300)
        x = (_unit(r, 300) * (CAVITY_RADIUS - depth)[:, None]).astype(F)
        return x, y
    if name in ("tiny", "underflow", "huge"):   # d2 in the denormal range; d2 that underflows to 0 for every pair; d2 near the top of the range (and infinite for far pairs)
        scale = {"tiny": 1e-20, "underflow": 1e-30, "huge": 3e19}[name]
        return (_uniform(400, 30).astype(np.float64) * scale).astype(F), (_uniform(m8 + 9, 31).astype(np.float64) * scale).astype(F)
    if name == "ulps_20":                       # a box 64 ulps wide at 2^20: neighbouring floats
        return (2.0 ** 20 + 0.125 * r.integers(0, 64, (400, 3))).astype(F), (2.0 ** 20 + 0.125 * r.integers(0, 64, (m8 + 9, 3))).astype(F)
    if name == "ulps_23":                       # a box 8 ulps wide at 2^23: fewer floats than cells
        return (2.0 ** 23 + r.integers(0, 8, (400, 3))).astype(F), (2.0 ** 23 + r.integers(0, 8, (m8 + 9, 3))).astype(F)
    if name == "aniso":                         # extents 10^12 apart
        scale = np.array([1e6, 1.0, 1e-6])
        return (_uniform(400, 32).astype(np.float64) * scale).astype(F), (_uniform(m8 + 9, 33).astype(np.float64) * scale).astype(F)
    if name == "shell":                         # a hollow surface cloud: 16 384 points on the unit sphere, queries on rays from the centre, from the centre itself to
        y = _unit(r, 16384).astype(F)           # outside the sphere, and five exactly at the centre
        x = np.concatenate([_unit(r, 200) * np.linspace(0.0, 1.2, 200)[:, None], np.zeros((5, 3))]).astype(F)
        return x, y
    if name == "symmetric":                     # the 48 signed permutations of (0.75, 0.5, 0.25), equidistant from the centre (0.875, exact in float32 in any order of
        import itertools                        # the sum), among 1024 others near the corners of the box [-0.8, 0.8]^3; queries at the centre and within 0.01 of it
        ring = np.array([[s0 * p[0], s1 * p[1], s2 * p[2]] for p in itertools.permutations((0.75, 0.5, 0.25)) for s0 in (-1, 1) for s1 in (-1, 1) for s2 in (-1, 1)])
        corner = r.choice([-1.0, 1.0], (m8, 3))
        others = corner * (0.8 - r.uniform(0.0, 0.04, (m8, 3)))
        others[:8] = [[s0 * 0.8, s1 * 0.8, s2 * 0.8] for s0 in (-1, 1) for s1 in (-1, 1) for s2 in (-1, 1)]
        y = np.concatenate([ring, others])[r.permutation(48 + m8)].astype(F)
        x = np.concatenate([np.zeros((1, 3)), r.uniform(-0.01, 0.01, (69, 3))]).astype(F)
        return x, np.ascontiguousarray(y)
    raise KeyError(name)


def symmetric_ring(y):
    """the indices of the 48 equidistant candidates of the case "symmetric": those whose coordinates are a signed permutation of (0.75, 0.5, 0.25)"""
    return np.nonzero((np.sort(np.abs(y), axis=1) == np.array([0.25, 0.5, 0.75], F)).all(1))[0]


# ---- the scan's passes: m on both sides of a change of res at which the number of scan chunks (2048 cells each) changes - from one chunk to two at res 13, and from
# 1024 to 1025 at res 128, where k_grid_scan_top's lanes first take more than one chunk each.  Not in CASES: the definition in numpy takes ten seconds at 4 M points.

SCAN_PASSES = {"12": ("scan_12_13", 13, -1), "13": ("scan_12_13", 13, 0), "127": ("scan_127_128", 128, -1), "128": ("scan_127_128", 128, 0)}
_SCAN = {}


def scan_pass(which, plan):
    """(x, y, index, dist2, stats) by the restatement for one side of a change of res: 257 uniform queries, m uniform candidates; computed once (do not modify)"""
    if which not in _SCAN:
        _name, res, off = SCAN_PASSES[which]
        m = _m_for_res(plan, res) + off
        x, y = _uniform(257, 300 + res), _uniform(m, 400 + res - off)
        p = plan(len(x), m)
        assert p.res == res + off
        _SCAN[which] = (x, y) + nearest(x, y, p.res, p.max_shells)
    return _SCAN[which]


WELL_SPREAD = ("uniform", "lattice", "bunny")                # the fallback's share must stay at or under FALLBACK_CAP (and "sampled", which the GPU test draws)
CAVITIES = tuple("cavity_%d" % k for k in CAVITY_BUDGETS)
GEOMETRY = ("tiny", "underflow", "huge", "ulps_20", "ulps_23", "aniso", "shell", "symmetric")
MUST_FALL_BACK = ("outside_far", "clusters") + CAVITIES + ("shell", "aniso", "underflow", "symmetric")                # the fallback must take some queries
CASES = ("uniform", "lattice", "tie_far_low", "tie_near_low", "copies", "identical_y", "same", "planar", "collinear", "far", "outside_near", "outside_far", "clusters", "hub",
         "bunny") + CAVITIES + GEOMETRY
FALLBACK_CAP = 0.05

_REF = {}


def reference(name, plan):
    """(x, y, index, dist2, stats) of a named case by the restatement, computed once and shared (do not modify)"""
    if name not in _REF:
        x, y = case(name, plan)
        p = plan(len(x), len(y))
        _REF[name] = (x, y) + nearest(x, y, p.res, p.max_shells)
    return _REF[name]
