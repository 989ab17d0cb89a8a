"""An independent reading of the Chamfer distance (include/psdr_hip.h states the definition; psdr_jit_amd/chamfer.py and csrc/hip/chamfer.hip implement it): numpy only,
shares no code with the package.

nearest(x, y) is the definition's scan in float32, in chunks of rows: d2 = (dx dx + dy dy) + dz dz with every operation a numpy float32 operation - one rounding each,
the definition's order - and argmin, which returns the first (lowest) index of the minimum.  The device must equal it bit for bit, indices and distances.

evaluate(x, y, idx_xy, idx_yx, weights, squared, dtype) gives the two direction means, the loss and the gradients through GIVEN indices (they are constants), in float64
or, with dtype=np.float32, the same statements in float32 with numpy's own summation order (pairwise np.sum for the means, np.add.at in element order for the gathered
part).  That float32 evaluation is the yardstick of the accuracy rule (tests/meshreg_ref.py says why it has this form):

    e_gpu = max |device - float64|,  e_32 = max |float32 checker - float64|,  G = max |float64|,  u = 2^-24:      e_gpu <= 4 max(e_32, u G)

The named cases take the package's launch_plan as an argument and put their sizes on its boundaries; nothing here is a hard-coded copy of the plan."""
import numpy as np

import subdiv_ref as sref

U = 2.0 ** -24
CHUNK = 1 << 22          # pairs per chunk of nearest()


def nearest(x, y):
    """(index int32 [N], dist2 float32 [N]): for every x_i the lowest j minimising d2(i, j), float32, the definition's operation order"""
    x, y = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32)
    n, m = len(x), len(y)
    idx, d2 = np.empty(n, np.int32), np.empty(n, np.float32)
    rows = max(1, CHUNK // m)
    y0, y1, y2 = y[None, :, 0], y[None, :, 1], y[None, :, 2]
    for r in range(0, n, rows):
        c = x[r:r + rows]
        dx, dy, dz = c[:, 0:1] - y0, c[:, 1:2] - y1, c[:, 2:3] - y2
        d = (dx * dx + dy * dy) + dz * dz
        assert d.dtype == np.float32
        k = d.argmin(1)
        idx[r:r + rows] = k
        d2[r:r + rows] = d[np.arange(len(c)), k]
    return idx, d2


def nearest_expansion(x, y):
    """the index the expansion form |x|^2 + |y|^2 - 2 x.y gives in float32: what the definition rules out (only to show that a case tells the two apart)"""
    x, y = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32)
    d = (x * x).sum(1)[:, None] + (y * y).sum(1)[None, :] - np.float32(2) * (x @ y.T)
    return d.argmin(1).astype(np.int32)


def _direction(p, o, idx, w, squared, T):
    """one direction, p -> o through idx: (mean of rho, d / dp [len(p), 3], d / do [len(o), 3]) with the weight w in the gradients only"""
    p, o = p.astype(T), o.astype(T)
    diff = p - o[idx]
    s = (diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]) + diff[:, 2] * diff[:, 2]
    n = len(p)
    if squared:
        val = s
        k = np.full(n, T(2.0 * w / n))
    else:
        val = np.sqrt(s)
        pos = s > 0
        k = np.where(pos, T(1.0 * w / n) / np.where(pos, val, T(1)), T(0))
    own = k[:, None] * diff
    other = np.zeros((len(o), 3), T)
    np.add.at(other, idx, -own)                    # in ascending element order: the device's order
    return T(val.sum() / T(n)), own.astype(T), other


def evaluate(x, y, idx_xy, idx_yx, weights=(1.0, 1.0), squared=True, dtype=np.float64):
    """-> {"terms": (mean_xy, mean_yx), "loss", "gx", "gy"}, every operation in `dtype`; a direction of weight 0 (or whose indices are None) is left out and reports 0"""
    T = dtype
    x, y = np.asarray(x), np.asarray(y)
    terms, loss = [T(0), T(0)], None
    gx, gy = None, None
    if weights[0] > 0:
        t, own, other = _direction(x, y, np.asarray(idx_xy, np.int64), weights[0], squared, T)
        terms[0], loss, gx, gy = t, T(weights[0]) * t, own, other
    if weights[1] > 0:
        t, own, other = _direction(y, x, np.asarray(idx_yx, np.int64), weights[1], squared, T)
        terms[1] = t
        loss = T(weights[1]) * t if loss is None else loss + T(weights[1]) * t
        gx, gy = (other, own) if gx is None else (gx + other, gy + own)
    if gx is None:
        loss, gx, gy = T(0), np.zeros((len(x), 3), T), np.zeros((len(y), 3), T)
    return {"terms": tuple(terms), "loss": T(loss), "gx": gx, "gy": gy}


def ratio(dev, f32, f64):
    """e_gpu / max(e_32, u G) (0 when everything is exactly 0), and its parts"""
    dev, f32, f64 = (np.asarray(a, np.float64) for a in (dev, f32, f64))
    e_gpu, e_32, G = np.abs(dev - f64).max(), np.abs(f32 - f64).max(), np.abs(f64).max()
    yard = max(e_32, U * G)
    return (0.0 if e_gpu == 0 else e_gpu / yard if yard > 0 else np.inf), e_gpu, e_32, G


# ---- the plan's boundaries, read from the plan

def narrow_max(plan):
    """the largest n that gets the queries_per_lane of n = 1 (bisection over the plan; the plan's queries_per_lane is monotone in n)"""
    q1 = plan(1, 1).queries_per_lane
    lo, hi = 1, 1 << 26
    if plan(hi, 1).queries_per_lane == q1:
        return hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if plan(mid, 1).queries_per_lane == q1 else (lo, mid)
    return lo


def first_long_slice(plan, n):
    """the smallest m at which a slice of the scan of n queries holds more than one tile"""
    tile = plan(n, 1).tile
    lo, hi = 1, 1 << 26
    assert plan(n, hi).slice_len > tile
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if plan(n, mid).slice_len > tile else (mid, hi)
    return hi


def query_sizes(plan):
    """N on the plan's edges: 1, the wave's 63 .. 65, one workgroup's queries +- 1 for every queries_per_lane the plan uses, the switch between them +- 1"""
    nm = narrow_max(plan)
    out = {1, 63, 64, 65}
    for n in (1, nm, nm + 1):
        if n <= 1 << 26:
            w = 256 * plan(n, 1).queries_per_lane
            out |= {w - 1, w, w + 1, 2 * w + 1}
    if nm < 1 << 20:
        out |= {nm - 1, nm, nm + 1}
    return sorted(out)


def candidate_sizes(plan):
    """M on the plan's edges for few queries: 1, tile - 1 .. tile + 1, two tiles +- 1, and three tiles + 1 (at least three slices)"""
    t = plan(1, 1).tile
    return [1, t - 1, t, t + 1, 2 * t - 1, 2 * t + 1, 3 * t + 1]


# ---- the clouds

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


def case(name, plan):
    """(x, y) float32 of a named case; `plan` is the package's launch_plan"""
    t = plan(1, 1).tile
    if name == "generic":                           # three slices of one tile each and a partial fourth, more than one workgroup of queries
        return _uniform(700, 1), _uniform(3 * t + 5, 2)
    if name == "wide":                              # the wide scan: several queries per lane, a last workgroup that is partly empty
        n = narrow_max(plan) + 300
        return _uniform(n, 3), _uniform(2 * t + 77, 4)
    if name in ("last", "first"):                   # every query's nearest is the last candidate of the last partial tile / candidate 0
        x = (np.float32(0.25) + np.float32(0.01) * _uniform(300, 5)).astype(np.float32)
        y = _uniform(3 * t + 5, 6, 2.0, 3.0)
        y[-1 if name == "last" else 0] = np.float32(0.25)
        return x, y
    if name == "identical_y":                       # all of y one point: every index is 0
        return _uniform(300, 7), np.repeat(_uniform(1, 8), 2 * t + 3, 0)
    if name == "same":                              # x is y: every distance 0 and a(i) = i
        x = _uniform(t + 300, 9)
        return x, x.copy()
    if name == "lattice":                           # coordinates in multiples of 2^-6 on an 8^3 lattice: many exact ties
        r = np.random.default_rng(10)
        return (r.integers(0, 8, (700, 3)) / 64.0).astype(np.float32), (r.integers(0, 8, (2 * t + 500, 3)) / 64.0).astype(np.float32)
    if name == "far":                               # coordinates around 1000 with a spacing of 1e-3: the expansion form fails here
        r = np.random.default_rng(11)
        x = (1000.0 + 1e-3 * r.integers(-40, 40, (500, 3)) + 2e-4 * r.uniform(-1, 1, (500, 3))).astype(np.float32)
        y = (1000.0 + 1e-3 * r.integers(-40, 40, (3 * t - 7, 3)) + 2e-4 * r.uniform(-1, 1, (3 * t - 7, 3))).astype(np.float32)
        return x, y
    if name == "bunny":                             # the bunny's vertices against a jittered copy
        v, _f = bunny()
        return v, (v + np.random.default_rng(12).normal(0.0, 0.01, v.shape)).astype(np.float32)
    if name == "one_query":                         # N = 1 and M large: all slices, one query; slices longer than a tile
        m = first_long_slice(plan, 1)
        length = plan(1, m).slice_len
        m = length * (-(-m // length) + 1) + 1      # slice_len k + 1 beyond that size: a last slice of one candidate
        return _uniform(1, 13), _uniform(m, 14)
    if name == "one_candidate":                     # N large and M = 1
        return _uniform(narrow_max(plan) * 4 + 3, 15), _uniform(1, 16)
    if name == "hub":                               # 300 points of y round x_0, more than a workgroup's lanes: b(j) = 0 for all of them
        x = np.concatenate([np.zeros((1, 3)), _uniform(40, 17, 4.0, 5.0)]).astype(np.float32)
        y = np.concatenate([0.3 * _uniform(300, 18), _uniform(30, 19, 4.0, 5.0)]).astype(np.float32)
        return x, y
    raise KeyError(name)


CASES = ("generic", "wide", "last", "first", "identical_y", "same", "lattice", "far", "bunny", "one_query", "one_candidate", "hub")

_REF = {}


def reference(name, plan):
    """(x, y, idx_xy, d2_xy, idx_yx, d2_yx) of a named case, computed once and shared (do not modify)"""
    if name not in _REF:
        x, y = case(name, plan)
        _REF[name] = (x, y) + nearest(x, y) + nearest(y, x)
    return _REF[name]
