"""The grid search, what can be checked without a GPU: grid_plan equals psdr_hip_chamfer_grid_plan over a sweep that holds every m at which res changes; the entry points
are declared, exported, listed and named in the stream contract under ABI 16, the operator list is what it was and nn_grid.h is among chamfer's dependencies; every entry
point refuses bad arguments before any device call and the Python surface before it looks for a device; the numpy restatement tests/pointgrid_ref.py - cell function,
build, shell walk, stopping rule, fallback - equals the definition's scan (chamfer_ref.nearest) bit for bit on every named case, with the fallback's share under the cap
on the well-spread cases and above zero where it must be; and a property sweep of the planes and of the cell function's monotonicity.

The cases that the GPU tests rely on for a particular path carry their conditions here (_conditions): the cavity cases reach every shell count up to a budget of 4, 5, 8,
12 and 16 shells with some queries certified by the last shell and some falling back, through slices of more than one tile from a budget of 8; the geometry cases really
have denormal, vanishing and near-overflow d2, boxes a few ulps wide, extents 10^12 apart, a hollow sphere, 48 exactly equidistant candidates.  The statistics change
when the budget is one shell off; the scan-pass sizes sit where the number of scan chunks changes (1 -> 2 and 1024 -> 1025); and check_build, which the GPU tests hold
the device's build to array by array, refuses each kind of wrong array."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import chamfer_ref as cref
import pointgrid_ref as pref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("psdr_hip_chamfer_grid_plan", "psdr_hip_chamfer_grid_build", "psdr_hip_chamfer_grid_nearest")
OPERATORS = ["precond", "adaptive", "denoise", "vdenoise", "subdiv", "msloss", "ssim", "meshreg", "chamfer", "sdf", "mtet", "latreg", "pointmesh"]
TOP = 1 << 26


@pytest.fixture(scope="module")
def psdr():
    import __graft_entry__
    __graft_entry__.build()
    import psdr_jit_amd
    return psdr_jit_amd


def _c_plan(L, n, m):
    o = [C.c_int32(), C.c_int32()] + [C.c_int64() for _ in range(6)] + [C.c_int32() for _ in range(4)]
    assert L.psdr_hip_chamfer_grid_plan(n, m, *[C.byref(v) for v in o]) == 0, L.psdr_hip_last_error().decode()
    return tuple(v.value for v in o)


def test_plan_python_equals_c(psdr):
    from psdr_jit_amd import cabi
    L, plan = cabi.lib(), psdr.grid_plan
    changes = pref.res_changes(plan, 256)                    # the smallest m of every res from 2 to 256
    assert len(changes) == 255 and changes == sorted(set(changes))
    ms = {1, 2, 63, 64, 65, 1000, 1023, 1024, 1025, 2503, 20000, 40962, 163842, 10 ** 6, TOP - 1, TOP}
    for m in changes:
        ms |= {m - 1, m, m + 1}
    seen = set()
    for m in sorted(ms):
        for n in (1, 1025, 65536, 65537, TOP):
            p = plan(n, m)
            assert (p.res, p.max_shells, p.cells, p.planes_at, p.begin_at, p.points_at, p.grid_words, p.work_words, p.fallback_groups, p.fallback_slices,
                    p.fallback_slice_len, p.lanes_per_query) == _c_plan(L, n, m), (n, m)
            assert (p.keys_len, p.list_len, p.stats_len) == (n, n, 2) and p.lanes_per_query == (8 if n <= 65536 else 1)
        assert 1 <= p.res <= 256 and p.cells == p.res ** 3 + 1 and p.max_shells == min(16, max(4, p.res // 4))
        assert p.res == 256 or 2 * (p.res + 1) ** 3 > m
        assert p.res == 1 or 2 * p.res ** 3 <= m
        # the blob's parts follow each other without overlap, the last two aligned to 4 words; the fallback's slices tile [0, m) and none is empty
        assert p.planes_at >= 16 and p.begin_at >= p.planes_at + 6 * p.res and p.points_at >= p.begin_at + p.cells and p.grid_words == p.points_at + 4 * m
        assert p.begin_at % 4 == 0 and p.points_at % 4 == 0 and p.grid_words < 2 ** 31
        assert p.work_words >= 8 + 2 * m + -(-p.cells // 2048)
        assert p.fallback_slice_len % 1024 == 0 and (p.fallback_slices - 1) * p.fallback_slice_len < m <= p.fallback_slices * p.fallback_slice_len and p.fallback_slices <= 32
        seen.add(p.res)
    assert seen == set(range(1, 257))
    assert [plan(1, m).res for m in (1, 15, 16, 53, 54, 127, 128, 1023, 1024)] == [1, 1, 2, 2, 3, 3, 4, 7, 8]
    for n, m in ((0, 1), (1, 0), (-1, 5), (TOP + 1, 1), (1, TOP + 1)):
        with pytest.raises(ValueError):
            plan(n, m)


def test_entry_points_declared_exported_listed(psdr):
    from psdr_jit_amd import build, cabi
    with open(os.path.join(ROOT, "include", "psdr_hip.h")) as fh:
        text = fh.read()
    L = cabi.lib()
    contract = text[text.index("THE STREAM CONTRACT"):text.index("const char *psdr_hip_last_error")]
    for name in NEW:
        assert re.search(r"^int\s+%s\s*\(" % name, text, re.M), "%s is not declared in include/psdr_hip.h" % name
        assert hasattr(L, name), "libpsdr_hip.so does not export %s" % name
        assert name in cabi.SYMBOLS
        assert getattr(L, name).argtypes is not None, "%s has no argtypes" % name
        assert name in contract
    assert re.search(r"#define\s+PSDR_HIP_ABI_VERSION\s+16\b", text)
    assert L.psdr_hip_abi_version() == 16
    for name in ("PointGrid", "grid_plan", "GridPlan", "nearest_points", "ChamferDistance"):
        assert hasattr(psdr, name)
    assert [u[0] for u in build.OPERATOR_UNITS] == OPERATORS
    units = {u[0]: u for u in build.hip_units()}
    deps = {os.path.relpath(d, ROOT) for d in units["chamfer"][3]}
    hip = os.path.join("psdr_jit_amd", "csrc", "hip")
    assert {os.path.join(hip, "nn_grid.h"), os.path.join(hip, "nn_scan.h"), os.path.join(hip, "op_common.h"), os.path.join("include", "psdr_hip.h")} <= deps
    assert os.path.join(ROOT, hip, "nn_grid.h") in build.HIP_DEPS
    # the d2 statement and the keys are the scan's: the grid's header uses them and holds no copy
    with open(os.path.join(ROOT, hip, "nn_grid.h")) as fh:
        grid_h = fh.read()
    assert "pair_d2(" in grid_h and "pack_key(" in grid_h and "__device__ __forceinline__ float pair_d2" not in grid_h and "pack_key(float" not in grid_h


def test_every_entry_point_refuses_bad_arguments_before_any_device_call(psdr):
    """no GPU is visible here: a call that reached the device would fail with a HIP error, not with the entry point's own message.  The non-NULL device pointers are host
    addresses that a refused call never reads."""
    from psdr_jit_amd import cabi
    L = cabi.lib()
    host = np.zeros(256, dtype=np.int64)
    p = [host.ctypes.data + 64 * i for i in range(20)]

    def refused(rc, name, word):
        msg = L.psdr_hip_last_error().decode()
        assert rc != 0 and msg.startswith(name + ":") and word in msg and "hip" not in msg[len(name):].lower(), (name, word, rc, msg)

    name = "psdr_hip_chamfer_grid_plan"
    new = lambda: [C.c_int32(), C.c_int32()] + [C.c_int64() for _ in range(6)] + [C.c_int32() for _ in range(4)]
    for n, m, word in ((0, 1, "n = 0"), (1, 0, "m = 0"), (TOP + 1, 1, "n = "), (1, -3, "m = -3"), (1, TOP + 1, "m = ")):
        refused(L.psdr_hip_chamfer_grid_plan(n, m, *[C.byref(v) for v in new()]), name, word)
    for k in range(12):
        args = [C.byref(v) for v in new()]
        args[k] = None
        refused(L.psdr_hip_chamfer_grid_plan(4, 4, *args), name, "NULL")
    plan = psdr.grid_plan(4, 4)
    name = "psdr_hip_chamfer_grid_build"
    fn = L.psdr_hip_chamfer_grid_build
    for m, word in ((0, "m = 0"), (-2, "m = -2"), (TOP + 1, "m = ")):
        refused(fn(p[0], m, p[1], 1 << 40, p[2], 1 << 40, None), name, word)
    for k in range(3):
        args = [p[0], p[1], p[2]]
        args[k] = None
        refused(fn(args[0], 4, args[1], plan.grid_words, args[2], plan.work_words, None), name, "NULL")
    refused(fn(p[0], 4, p[1], plan.grid_words - 1, p[2], plan.work_words, None), name, "grid_words")
    refused(fn(p[0], 4, p[1], plan.grid_words, p[2], plan.work_words - 1, None), name, "work_words")
    refused(fn(p[0], 4, p[1], 0, p[2], plan.work_words, None), name, "grid_words")
    name = "psdr_hip_chamfer_grid_nearest"
    fn = L.psdr_hip_chamfer_grid_nearest
    for n, m, word in ((0, 1, "n = 0"), (1, 0, "m = 0"), (TOP + 1, 1, "n = "), (1, TOP + 1, "m = ")):
        refused(fn(p[0], n, p[1], m, p[2], 1 << 40, p[3], p[4], p[5], p[6], p[7], None), name, word)
    for k in range(8):
        a = [p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7]]
        a[k] = None
        refused(fn(a[0], 4, a[1], 4, a[2], plan.grid_words, a[3], a[4], a[5], a[6], a[7], None), name, "NULL")
    refused(fn(p[0], 4, p[1], 4, p[2], plan.grid_words - 1, p[3], p[4], p[5], p[6], p[7], None), name, "grid_words")
    assert not host.any()


def test_python_surface_refusals(psdr):
    """wrong arguments are a ValueError before a device is looked for (there is none here)"""
    import torch
    good = torch.zeros(5, 3)
    for search in ("auto", "tree", None, 1, "Grid"):
        with pytest.raises(ValueError):
            psdr.nearest_points(good, good, search=search)
        with pytest.raises(ValueError):
            psdr.ChamferDistance(search=search)
    cd = psdr.ChamferDistance(search="grid")
    assert cd.search == "grid" and psdr.ChamferDistance().search == "scan"
    cd.search = "auto"                                        # a plain attribute, read at every call
    with pytest.raises(ValueError):
        cd(good, good)
    cd.search = "grid"
    bad_points = (torch.zeros(5, 2), torch.zeros(0, 3), torch.zeros(5, 3, dtype=torch.int32), torch.zeros(5), np.zeros((4, 3), np.int64))
    for bad in bad_points:
        with pytest.raises(ValueError):
            psdr.PointGrid(bad)
        for args in ((bad, good), (good, bad)):
            with pytest.raises(ValueError):
                psdr.nearest_points(*args, search="grid")
            with pytest.raises(ValueError):
                cd.value_and_grad(*args)
    with pytest.raises(ValueError):
        psdr.nearest_points(good, good, return_stats=True)     # the scan keeps no statistics

    def fake(points, blob):
        g = psdr.PointGrid.__new__(psdr.PointGrid)
        g.points, g.blob, g.num_points = points, blob, int(points.shape[0]) if points.dim() else 0
        return g

    words = psdr.grid_plan(1, 5).grid_words
    on_host = fake(torch.zeros(5, 3), torch.zeros(words, dtype=torch.int32))                  # another device: the host
    wrong_dtype = fake(torch.zeros(5, 3, dtype=torch.float64), torch.zeros(words, dtype=torch.int32))
    wrong_blob = fake(torch.zeros(5, 3), torch.zeros(words, dtype=torch.float32))
    wrong_shape = fake(torch.zeros(5, 4), torch.zeros(words, dtype=torch.int32))
    for g in (on_host, wrong_dtype, wrong_blob, wrong_shape):
        with pytest.raises(ValueError):
            psdr.nearest_points(good, g)
        with pytest.raises(ValueError):
            cd(good, good, y_grid=g)
        with pytest.raises(ValueError):
            cd.value_and_grad(good, good, y_grid=g)
    with pytest.raises(ValueError):
        cd(good, good, y_grid=good)                            # not a PointGrid
    with pytest.raises(ValueError):
        psdr.nearest_points(torch.zeros(5, 2), on_host)


def _check_case(psdr, name):
    x, y, idx, d2, st = pref.reference(name, psdr.grid_plan)
    want_i, want_d = cref.nearest(x, y)
    assert np.array_equal(idx, want_i) and d2.tobytes() == want_d.tobytes(), name
    return x, y, st


@pytest.mark.parametrize("name", pref.CASES)
def test_restatement_is_the_definition(psdr, name):
    x, y, st = _check_case(psdr, name)
    share = st["fallback"] / len(x)
    print("%s: n = %d, m = %d, res = %d, dims %s, fallback %d (%.2f %%), pairs per query %.1f by the walk, shells %s" %
          (name, len(x), len(y), st["grid"].res, st["grid"].dim, st["fallback"], 100 * share, st["walk_pairs"] / len(x), np.bincount(st["shells"]).tolist()))
    if name in pref.WELL_SPREAD:
        assert share <= pref.FALLBACK_CAP
        assert st["walk_pairs"] < 0.5 * len(x) * len(y)          # (the grid decides: far fewer pairs than the scan's)
    if name in pref.MUST_FALL_BACK:
        assert st["fallback"] > 0
    if name in ("tie_far_low", "tie_near_low"):                  # the tie is real, and the lower index wins wherever it lies
        d = cref.nearest(x, y)[1]
        assert (d == np.float32(0.0625)).all() and (pref.reference(name, psdr.grid_plan)[2] == 5).all()
    if name in ("planar", "collinear"):
        assert st["grid"].dim.count(1) == (1 if name == "planar" else 2)
    _conditions(psdr, name, x, y, st)


def _conditions(psdr, name, x, y, st):
    """what each of the cavity and geometry cases is for: a case that stops exercising it fails here, on the CPU, and does not pass silently on the GPU"""
    from psdr_jit_amd import pointgrid
    n, m = len(x), len(y)
    p = psdr.grid_plan(n, m)
    idx, d2 = pref.reference(name, psdr.grid_plan)[2:4]
    seen = np.bincount(st["shells"], minlength=p.max_shells + 1)
    assert st["grid"].res == p.res and len(seen) == p.max_shells + 1
    if name in pref.CAVITIES:
        k = int(name.split("_")[1])
        assert p.max_shells == k and p.res == 4 * k and m == 2 * p.res ** 3 and psdr.grid_plan(n, m - 1).res == p.res - 1
        assert (seen[2:] > 0).all(), "not every shell count from 2 to %d occurs: %s" % (k, seen.tolist())
        assert 0 < st["fallback"] < n
        assert st["fell"].sum() == st["fallback"] and (st["shells"][st["fell"]] == k).all()          # the fallback takes a query after exactly max_shells shells
        assert ((st["shells"] == k) & ~st["fell"]).any()                                             # ... and not one that the last shell certified
        if k >= 8:                                   # slices of more than one LDS tile, all 32 of them where the tiles divide evenly: 64, 216 and 512 tiles make
            assert pointgrid.FALLBACK_SLICES == 32 and p.fallback_slice_len > pointgrid.TILE             # 32 x 2, 31 x 7 (the last slice short) and 32 x 16
            assert (p.fallback_slices, p.fallback_slice_len // pointgrid.TILE) == {8: (32, 2), 12: (31, 7), 16: (32, 16)}[k]
        else:
            assert p.fallback_slices < 32 and p.fallback_slice_len == pointgrid.TILE
    if name in pref.GEOMETRY and name not in ("shell", "symmetric"):
        assert (n, m) == (400, pref._m_for_res(psdr.grid_plan, 8) + 9)
    tiny = np.float32(2.0 ** -126)                                                                   # the smallest normal float32
    if name == "tiny":
        assert (d2 > 0).all() and (d2 < tiny).all() and st["fallback"] == 0
    if name == "underflow":
        assert (np.abs(y).max(0) > tiny).all() and not d2.any() and not idx.any() and st["fallback"] == n
        dx = x[:, None, 0] - y[None, :, 0]
        assert not (dx * dx).any()                                                                   # every pair, not only the winners
    if name == "huge":
        assert np.isfinite(d2).all() and d2.max() > 1e37                                             # (the largest float32 is 3.4e38)
        with np.errstate(over="ignore"):
            assert np.isinf((x[0] - y) ** 2).any()                                                  # (far pairs overflow: an infinite d2 must never win)
    if name in ("ulps_20", "ulps_23"):
        at = np.float32(2.0 ** (20 if name == "ulps_20" else 23))
        for a in range(3):
            v = np.unique(y[:, a])
            assert (np.diff(v) == np.spacing(at)).all() and v[0] == at and len(v) == (64 if name == "ulps_20" else 8)
        assert st["grid"].dim == [p.res] * 3
        if name == "ulps_23":
            assert p.res == 8 and (d2 == 0).sum() > n // 2                                           # as many floats along an axis as cells: 512 distinct points
    if name == "aniso":
        extent = st["grid"].hi - st["grid"].lo
        assert extent[0] / extent[2] > 1e11 and st["fallback"] == n and st["grid"].dim == [p.res] * 3
    if name == "shell":
        assert (n, m, p.res, p.max_shells) == (205, 16384, 20, 5)
        assert (seen[1:] > 0).all() and 0 < st["fallback"] < n and st["fell"][200:].all() and not x[200:].any()
    if name == "symmetric":
        ring = pref.symmetric_ring(y)
        assert n == 70 and len(ring) == 48 and st["fallback"] == n
        assert not x[0].any() and d2[0] == np.float32(0.875) and idx[0] == ring.min()
        d = (x[0] - y[ring]) ** 2
        assert ((d[:, 0] + d[:, 1]) + d[:, 2] == np.float32(0.875)).all()                            # equidistant from the centre, exactly
        assert np.isin(idx, ring).all() and len(set(idx.tolist())) > 8                               # off the centre the winner moves round the ring


def test_the_statistics_pin_the_shell_budget(psdr):
    """the device's (fallback, pairs) are asked to EQUAL the restatement's at the plan's max_shells: on cavity_8 a budget of one shell less or one more gives other
    figures, so that equality does pin the budget (and "not certified after exactly max_shells shells goes to the list")"""
    x, y, _idx, _d2, st = pref.reference("cavity_8", psdr.grid_plan)
    p = psdr.grid_plan(len(x), len(y))
    assert p.max_shells == 8
    at = {8: (st["fallback"], st["pairs"])}
    for shells in (7, 9):
        idx, d2, other = pref.nearest(x, y, p.res, shells)
        at[shells] = (other["fallback"], other["pairs"])
        assert np.array_equal(idx, pref.reference("cavity_8", psdr.grid_plan)[2])                    # (the results do not depend on the budget)
    print("cavity_8: (fallback, pairs) at a budget of 7, 8, 9 shells: %s" % [at[k] for k in (7, 8, 9)])
    assert at[7] != at[8] and at[9] != at[8] and at[7][0] >= at[8][0] >= at[9][0]


@pytest.mark.parametrize("which", sorted(pref.SCAN_PASSES, key=int))
def test_scan_passes_restatement(psdr, which):
    """m on both sides of the change of res 12 -> 13 (one chunk of 2048 cells, then two) and 127 -> 128 (1024 chunks, then 1025: the first size at which a lane of the
    second scan level takes more than one chunk sum): the chunk counts read from the plan, and the restatement against the definition - on 16 of the 257 queries at
    four million candidates, to keep numpy's scan short"""
    from psdr_jit_amd import pointgrid
    plan = psdr.grid_plan
    x, y, idx, d2, st = pref.scan_pass(which, plan)
    _name, res, off = pref.SCAN_PASSES[which]
    m = len(y)
    assert len(x) == 257 and plan(1, m).res == res + off == int(which) and plan(1, m - off).res == res and plan(1, m - off - 1).res == res - 1
    chunks = pref.scan_chunks(plan, m, pointgrid.WORK_HEAD)
    assert chunks == -(-((res + off) ** 3 + 1) // pointgrid.SCAN_CHUNK)
    assert {"12": chunks == 1, "13": chunks == 2, "127": 1 < chunks <= 1024, "128": chunks > 1024}[which], chunks
    if which == "128":
        assert m == 4194304 and chunks == 1025
    take = slice(None) if m < 100000 else slice(0, 257, 17)
    assert len(x[take]) in (257, 16)
    want_i, want_d = cref.nearest(x[take], y)
    assert np.array_equal(idx[take], want_i) and d2[take].tobytes() == want_d.tobytes()
    print("scan pass at res %s: m = %d, %d chunks, fallback %d, pairs %d, shells %s" % (which, m, chunks, st["fallback"], st["pairs"], np.bincount(st["shells"]).tolist()))


class _Built:
    """what check_build reads of a PointGrid, made from the restatement's Grid: numpy arrays in the blob's layout"""

    def __init__(self, G):
        self.points = G.y.copy()
        self.box = np.concatenate([G.lo, G.inv, G.width]).astype(np.float32)
        self.dims = np.array(G.dim, np.int32)
        self.planes = np.stack([np.stack([G.up[a], G.down[a]]) for a in range(3)]).astype(np.float32).ravel()
        self.cell_begin = G.begin.astype(np.int32)
        order = G.order.copy()
        for c in np.nonzero(np.diff(G.begin) > 1)[0]:                                                # another order inside every cell: it is not defined
            order[G.begin[c]:G.begin[c + 1]] = order[G.begin[c]:G.begin[c + 1]][::-1]
        self.sorted = np.concatenate([G.y[order].view(np.int32), order.astype(np.int32)[:, None]], 1)


def test_check_build_tells_a_wrong_array(psdr):
    """the helper the GPU tests hold the device's build to: it accepts the restatement's own arrays with the cells' contents reordered, and refuses one wrong plane, one
    wrong infinity, one wrong cell_begin entry in the middle, a wrong constant, a row with another point's coordinates and two indices swapped across cells"""
    G = pref.reference("uniform", psdr.grid_plan)[4]["grid"]
    pref.check_build(_Built(G), G)
    mid = len(G.begin) // 2

    def plane(b):
        b.planes[G.res + 3] = np.nextafter(b.planes[G.res + 3], np.float32(np.inf))

    def infinity(b):
        assert b.planes[0] == -np.inf
        b.planes[0] = G.lo[0]

    def begin(b):
        b.cell_begin[mid] += 1

    def constant(b):
        b.box[4] = np.nextafter(b.box[4], np.float32(0))

    def row(b):
        b.sorted[5, 0] = b.sorted[6, 0] + 1

    def swapped(b):
        b.sorted[[0, -1]] = b.sorted[[-1, 0]]

    def dims(b):
        b.dims[1] = 1

    for spoil in (plane, infinity, begin, constant, row, swapped, dims):
        b = _Built(G)
        spoil(b)
        with pytest.raises(AssertionError):
            pref.check_build(b, G)


def test_restatement_on_small_sizes_and_sampled_points(psdr):
    """M on every change of res up to 8, +- 1, against a few N; and points drawn on the bunny (what SurfaceSampler draws, in numpy) stay under the fallback cap"""
    plan = psdr.grid_plan
    ms = sorted({m + d for m in [1] + pref.res_changes(plan) for d in (-1, 0, 1) if m + d >= 1})
    for m in ms:
        for n in (1, 65, 257):
            x, y = pref._uniform(n, 100 + n), pref._uniform(m, 200 + m)
            p = plan(n, m)
            idx, d2, _st = pref.nearest(x, y, p.res, p.max_shells)
            want_i, want_d = cref.nearest(x, y)
            assert np.array_equal(idx, want_i) and d2.tobytes() == want_d.tobytes(), (n, m)
    v, f = cref.bunny()
    pts = []
    for seed in (1, 2):
        face, bary = psdr.sample_surface(v, f, 20000, np.random.default_rng(seed))
        pts.append((bary.astype(np.float32)[:, :, None] * v[f[face]]).sum(1).astype(np.float32))
    p = plan(20000, 20000)
    idx, d2, st = pref.nearest(pts[0], pts[1], p.res, p.max_shells)
    print("sampled: res = %d, fallback %d of 20000, pairs per query %.1f, shells %s" % (p.res, st["fallback"], st["walk_pairs"] / 20000.0, np.bincount(st["shells"]).tolist()))
    assert st["fallback"] <= pref.FALLBACK_CAP * 20000
    want_i, want_d = cref.nearest(pts[0][::10], pts[1])
    assert np.array_equal(idx[::10], want_i) and d2[::10].tobytes() == want_d.tobytes()


def test_planes_and_monotone_cell_function():
    """a few thousand random (lo, extent, res): the plane found for k really has c(b) < k (upper) or c(b) > k (lower) - or is the infinity that certifies nothing - and the
    search nearly always finds one; c is monotone non-decreasing on sorted random floats, also beyond the box"""
    r = np.random.default_rng(0)
    found = total = 0
    for _ in range(3000):
        lo = np.float32(r.choice([0.0, 1.0, -1.0, 1000.0, -1e-3, 1e6]) + r.normal() * 10.0 ** r.integers(-3, 4))
        extent = np.float32(10.0 ** r.uniform(-4, 4))
        hi = np.float32(lo + extent)
        res = int(r.integers(1, 257))
        inv, width, dim = pref.axis_constants(lo, hi, res)
        assert dim in (1, res)
        for k in {1, dim // 2, dim - 1, int(r.integers(0, dim + 1))}:
            b = pref.plane(lo, hi, inv, width, dim, 0, k)
            if 1 <= k < dim:
                total += 1
                found += bool(np.isfinite(b))
                assert b == -np.inf or pref.cell_of(b, lo, inv, dim) < k
            else:
                assert b == -np.inf
            b = pref.plane(lo, hi, inv, width, dim, 1, k - 1)
            if 0 <= k - 1 < dim - 1:
                total += 1
                found += bool(np.isfinite(b))
                assert b == np.inf or pref.cell_of(b, lo, inv, dim) > k - 1
            else:
                assert b == np.inf
        v = np.sort(np.concatenate([r.uniform(lo - extent, hi + extent, 200), r.uniform(lo, hi, 200), [lo, hi, -np.inf, np.inf]]).astype(np.float32))
        c = pref.cell_of(v, lo, inv, dim)
        assert (np.diff(c) >= 0).all() and c.min() >= 0 and c.max() <= dim - 1
    print("planes found: %d of %d" % (found, total))
    assert total > 3000 and found >= 0.99 * total
