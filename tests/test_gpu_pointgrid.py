"""GPU tests of the grid search (psdr_jit_amd/pointgrid.py, csrc/hip/nn_grid.h): nearest_points(x, y, search="grid") against the definition's scan in numpy
(chamfer_ref.nearest) - both arrays, no tolerance - and, above 20 000 points, against search="scan", which tests/test_gpu_chamfer.py pins to the same definition.  Sizes
are read from grid_plan.

Bit comparisons alone could pass with every query in the fallback, without the grid ever deciding anything.  So every case also compares the device's statistics with the
numpy restatement's (tests/pointgrid_ref.py): the queries the fallback finished and the pairs tested are EQUAL - the walk tests every candidate of every cell of
every shell a query visits and the fallback m per listed query, whatever the lanes that share the query: well defined, so equality is asked everywhere, not a bound.  On the well-spread cases
the fallback's share is at most 5 %, on the far-away and between-clusters cases it is above zero.

"An exact copy of the winner in a neighbouring / a far cell" cannot exist in a grid - equal coordinates have equal cells - so the case "copies" holds exact copies at
other positions of the index order (same cell), and the ties across cells are the equidistant twins of tie_far_low / tie_near_low and the lattice's.

Beyond res 8 - 11 (tests/pointgrid_ref.py has the constructions, tests/test_pointgrid_cpu.py the conditions that keep each case on its path):
  cavity_4 .. cavity_16   a full box with a ball cut out, queries in the hollow at every depth: shell budgets 4, 5, 8, 12, 16 (res 16 .. 64, m up to 524 288), every shell
                          count up to the budget, the walk's column decomposition at s >= 5, the hand-over to the list after exactly max_shells shells, and from a
                          budget of 8 a fallback of 31 - 32 slices of 2 - 16 tiles
  tiny, underflow, huge, ulps_20, ulps_23, aniso, shell, symmetric
                          d2 denormal / 0 for every pair / up to 1e37 and infinite beyond; boxes 64 and 8 ulps wide; extents 10^12 apart; a hollow sphere with queries at
                          its centre; 48 candidates exactly equidistant from a query
  test_scan_passes        m on both sides of res 12 -> 13 and 127 -> 128: one, two, 1001 and 1025 chunks of the exclusive scan - the last the first size at which a lane
                          of the scan's second level takes more than one chunk sum - against search="scan" on the device
Every named case and every scan pass also holds the device's BUILD to the restatement's, array by array (_build: box, dims, every plane, every cell_begin entry, the
sorted rows and each cell's set of indices)."""
import numpy as np
import pytest

import chamfer_ref as cref
import pointgrid_ref as pref
from stream_cases import Slot, decoy_of, run_on_stream, run_plain

pytestmark = pytest.mark.gpu

QUERY_SIZES = (1, 63, 64, 65, 255, 256, 257, 1025)


@pytest.fixture(scope="module")
def psdr():
    import __graft_entry__
    __graft_entry__.build()
    import psdr_jit_amd
    return psdr_jit_amd


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _grid(psdr, x, y):
    """(index, dist2, (fallback, pairs)) of the device's grid search; x and y numpy arrays, or tensors that are on the device already"""
    import torch
    tensor = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    idx, d2, stats = psdr.nearest_points(tensor(x), tensor(y), search="grid", return_stats=True)
    assert idx.dtype == torch.int32 and d2.dtype == torch.float32 and stats.dtype == torch.int64 and stats.shape == (2,)
    assert idx.is_cuda and d2.is_cuda and stats.is_cuda and not idx.requires_grad and not d2.requires_grad
    return idx.cpu().numpy(), d2.cpu().numpy(), tuple(int(v) for v in stats.cpu())


def _same(psdr, x, y, what, want=None, stats=None):
    idx, d2, got = _grid(psdr, x, y)
    want_i, want_d = cref.nearest(x, y) if want is None else want
    assert idx.min() >= 0 and idx.max() < len(y)
    bad = np.nonzero((idx != want_i) | (d2.view(np.uint32) != want_d.view(np.uint32)))[0]
    assert bad.size == 0, "%s: %d of %d queries differ, first %d: device (%d, %r) definition (%d, %r)" % (what, bad.size, len(x), bad[0], idx[bad[0]], d2[bad[0]], want_i[bad[0]], want_d[bad[0]])
    if stats is None:
        p = psdr.grid_plan(len(x), len(y))
        stats = pref.nearest(x, y, p.res, p.max_shells)[2]
    print("%s: n = %d, m = %d: fallback %d (restatement %d), pairs %d (restatement %d)" % (what, len(x), len(y), got[0], stats["fallback"], got[1], stats["pairs"]))
    assert got == (stats["fallback"], stats["pairs"]), what
    return got


def test_sizes_on_every_change_of_res(psdr):
    """M on every change of res from 1 up to 8, +- 1, against N on the wave's and the workgroup's edges"""
    plan = psdr.grid_plan
    ms = sorted({m + d for m in [1] + pref.res_changes(plan) for d in (-1, 0, 1) if m + d >= 1})
    assert {plan(1, m).res for m in ms} == set(range(1, 9))
    for m in ms:
        y = pref._uniform(m, 200 + m)
        for n in QUERY_SIZES:
            _same(psdr, pref._uniform(n, 100 + n), y, "n %d m %d" % (n, m))


@pytest.mark.parametrize("name", pref.CASES)
def test_named_cases(psdr, name):
    x, y, idx, d2, stats = pref.reference(name, psdr.grid_plan)
    fallback, _pairs = _same(psdr, x, y, name, want=cref.nearest(x, y), stats=stats)
    if name in pref.WELL_SPREAD:
        assert fallback <= pref.FALLBACK_CAP * len(x)
    if name in pref.MUST_FALL_BACK:
        assert fallback > 0
    _build(psdr, y, stats["grid"], name)


def _build(psdr, y, G, what):
    """the device's build of y against the restatement's, array by array (pointgrid_ref.check_build); -> the PointGrid, its candidates on the device"""
    import torch
    grid = psdr.PointGrid(torch.from_numpy(y).cuda() if isinstance(y, np.ndarray) else y)
    p = grid.plan
    assert (p.res, grid.num_points) == (G.res, G.m) and grid.box.shape == (9,) and grid.dims.shape == (3,) and grid.planes.shape == (6 * p.res,)
    pref.check_build(grid, G, what)
    return grid


@pytest.mark.parametrize("which", sorted(pref.SCAN_PASSES, key=int))
def test_scan_passes(psdr, which):
    """m on both sides of the change of res 12 -> 13 (one chunk of 2048 cells in the exclusive scan, then two) and of 127 -> 128 (1024 chunks, then 1025: k_grid_scan_top's
    lanes take two chunk sums each for the first time): the build array by array, then the search against search="scan" on the device, the statistics the restatement's"""
    import torch
    from psdr_jit_amd import pointgrid
    x, y, _idx, _d2, stats = pref.scan_pass(which, psdr.grid_plan)
    chunks = pref.scan_chunks(psdr.grid_plan, len(y), pointgrid.WORK_HEAD)
    assert {"12": chunks == 1, "13": chunks == 2, "127": 1 < chunks <= 1024, "128": chunks > 1024}[which]
    yd = torch.from_numpy(y).cuda()                                           # (the candidates go to the device once)
    grid = _build(psdr, yd, stats["grid"], "res " + which)
    xd = torch.from_numpy(x).cuda()
    want = tuple(t.cpu().numpy() for t in psdr.nearest_points(xd, yd, search="scan"))
    _same(psdr, xd, yd, "res " + which, want=want, stats=stats)
    if which == "128":                                                        # a grid built before the call against the one _same built in its call: same bits, same statistics
        idx, d2, st = psdr.nearest_points(xd, grid, return_stats=True)
        assert _bits(idx.cpu().numpy()) == _bits(want[0]) and _bits(d2.cpu().numpy()) == _bits(want[1])
        assert tuple(int(v) for v in st.cpu()) == (stats["fallback"], stats["pairs"])


def test_chamfer_distance_at_a_budget_of_eight_shells(psdr):
    """cavity_8 (m = 65 536, n = 300, max_shells 8), both directions: x -> y walks up to eight shells and falls back through 32 slices of two tiles; y -> x builds a
    grid of 300 points (res 5) and searches it with 65 536 queries, the most that eight lanes share.  Loss, terms, both gradients and the nearest arrays equal the scan's byte for byte"""
    import torch
    x, y = pref.reference("cavity_8", psdr.grid_plan)[:2]
    assert psdr.grid_plan(len(x), len(y)).max_shells == 8 and psdr.grid_plan(len(y), len(x)).lanes_per_query == psdr.grid_plan(1, 1).lanes_per_query
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    scan = _eval(psdr.ChamferDistance((1.0, 0.5)), xd, yd)
    assert len(scan) == 8
    assert _eval(psdr.ChamferDistance((1.0, 0.5), search="grid"), xd, yd) == scan


def test_both_walks_round_the_switch_of_lanes_per_query(psdr):
    """the plan walks a query with a group of lanes up to some n and with one lane beyond: n on both sides of the switch, and named cases repeated to a size beyond it
    (the walk of a query does not depend on the others, so the statistics are the sums of the restatement's per-query figures), against search="scan" on the device"""
    import torch
    plan = psdr.grid_plan
    few = plan(1, 1).lanes_per_query
    lo, hi = 1, 1 << 26
    assert plan(hi, 1).lanes_per_query != few
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if plan(mid, 1).lanes_per_query == few else (lo, mid)
    for name, sizes in (("uniform", (lo, hi)), ("lattice", (hi,)), ("planar", (hi,)), ("hub", (hi,)), ("clusters", (hi + 63,))):
        x, y, _idx, _d2, st = pref.reference(name, plan)
        yd = torch.from_numpy(y).cuda()
        for n in sizes:
            assert plan(n, len(y)).lanes_per_query == (few if n <= lo else plan(hi, 1).lanes_per_query)
            take = np.arange(n) % len(x)
            big = np.ascontiguousarray(x[take])
            want = tuple(t.cpu().numpy() for t in psdr.nearest_points(torch.from_numpy(big).cuda(), yd, search="scan"))
            fell = int(st["fell"][take].sum())
            _same(psdr, big, y, "%s repeated to %d" % (name, n), want=want, stats={"fallback": fell, "pairs": int(st["walk_pairs_of"][take].sum()) + fell * len(y)})


def test_sampled_points_against_the_scan(psdr):
    """20 000 SurfaceSampler points against 20 000 others: compared with search="scan" on the device; the statistics with the restatement's on the device's points"""
    import torch
    v, f = cref.bunny()
    moved = (v + 0.05 * np.sin(3.0 * v[:, [1, 2, 0]])).astype(np.float32)
    x = psdr.SurfaceSampler(f, len(v), num_points=20000, seed=0).resample(v)(torch.from_numpy(v)).detach()
    y = psdr.SurfaceSampler(f, len(v), num_points=20000, seed=1).resample(moved)(torch.from_numpy(moved)).detach()
    want = tuple(t.cpu().numpy() for t in psdr.nearest_points(x, y, search="scan"))
    xn, yn = x.cpu().numpy(), y.cpu().numpy()
    fallback, pairs = _same(psdr, xn, yn, "sampled", want=want)
    assert fallback <= pref.FALLBACK_CAP * 20000 and pairs < 0.05 * 20000 * 20000


def test_non_finite_inputs_return_with_indices_in_range(psdr):
    x, y = pref._uniform(65, 40), pref._uniform(65, 41)
    x[3, 1], x[40, 0], y[7, 2], y[50, 1] = np.nan, np.inf, np.nan, -np.inf
    idx, d2, stats = _grid(psdr, x, y)
    assert idx.shape == (65,) and idx.min() >= 0 and idx.max() < 65 and 0 <= stats[0] <= 65


def _eval(cd, x, y, **kw):
    loss, gx, gy = cd.value_and_grad(x, y, **kw)
    return tuple(_bits(t.cpu().numpy()) for t in (loss, cd.terms, gx, gy) + tuple(t for t in cd.nearest if t is not None))


@pytest.mark.parametrize("squared", [True, False])
def test_chamfer_distance_keeps_the_bits_of_the_scan(psdr, squared):
    """loss, terms, both gradients and the nearest arrays, each direction alone and both together; a prebuilt grid of the target; ten calls; one grid, two x"""
    import torch
    x, y = pref.case("uniform", psdr.grid_plan)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    grid = psdr.PointGrid(yd)
    for weights in ((1.0, 0.5), (1.0, 0.0), (0.0, 1.0)):
        scan = _eval(psdr.ChamferDistance(weights, squared), xd, yd)
        cd = psdr.ChamferDistance(weights, squared, search="grid")
        assert _eval(cd, xd, yd) == scan
        assert _eval(cd, xd, yd, y_grid=grid) == scan
        assert _eval(psdr.ChamferDistance(weights, squared), xd, yd, y_grid=grid) == scan
    cd = psdr.ChamferDistance((1.0, 0.5), squared, search="grid")
    first = _eval(cd, xd, yd)
    assert all(_eval(cd, xd, yd) == first for _ in range(9))
    x2 = torch.from_numpy(pref._uniform(777, 55)).cuda()
    for q in (xd, x2):                                               # a grid built once serves two different x
        got = psdr.nearest_points(q, grid)
        want = psdr.nearest_points(q, yd)
        assert torch.equal(got[0], want[0]) and _bits(got[1].cpu().numpy()) == _bits(want[1].cpu().numpy())
    p = grid.plan
    assert grid.cell_begin.shape == (p.res ** 3 + 1,) and int(grid.cell_begin[-1]) == len(y) and int(grid.cell_begin[0]) == 0
    assert sorted(grid.sorted[:, 3].contiguous().view(torch.int32).cpu().tolist()) == list(range(len(y)))          # every candidate once, with its original index
    assert grid.dims.cpu().tolist() == [p.res] * 3 and grid.planes.shape == (6 * p.res,) and grid.box.shape == (9,)
    with pytest.raises(ValueError):
        cd(xd, yd[:-1], y_grid=grid)


@pytest.mark.parametrize("form", ("S", "default"))
def test_streams(psdr, form):
    """both forms of the delayed producer, with the inputs rolled along their first axis as decoys: on the build (PointGrid), on the search of a grid built before and of
    one built in the call, and on cd(x, y) with search="grid" plus its backward"""
    import torch
    x, y = pref.case("uniform", psdr.grid_plan)
    cd = psdr.ChamferDistance(weights=(1.0, 0.5), search="grid")
    sx, sy = Slot(torch, x), Slot(torch, y)
    fetch = lambda t: tuple(a.cpu().numpy() for a in t)
    call = lambda: cd.value_and_grad(sx.buf, sy.buf) + (cd.terms,) + cd.nearest
    base = run_plain(torch, [sx, sy], call, fetch)
    scan = psdr.ChamferDistance(weights=(1.0, 0.5))
    want = fetch(scan.value_and_grad(sx.buf, sy.buf) + (scan.terms,) + scan.nearest)
    assert all(_bits(a) == _bits(b) for a, b in zip(base, want))
    for k, (dx_, dy_) in enumerate(((decoy_of(x), y), (x, decoy_of(y)))):          # (each decoy is told apart: the rolled set's own gradient is rolled with it)
        decoy = fetch(cd.value_and_grad(torch.from_numpy(dx_).cuda(), torch.from_numpy(dy_).cuda()))
        assert _bits(decoy[1 + k]) != _bits(base[1 + k])
    S = torch.cuda.Stream()

    def autograd():                                      # (backward waits on the host for the engine's thread: no self-check)
        lx, ly = sx.buf.clone().requires_grad_(), sy.buf.clone().requires_grad_()
        cd(lx, ly).backward()
        return (lx.grad, ly.grad)
    got = run_on_stream(torch, S, form, [sx, sy], autograd, fetch, returns_early=False)
    assert _bits(got[0]) == _bits(base[1]) and _bits(got[1]) == _bits(base[2])
    got = run_on_stream(torch, S, form, [sx, sy], call, fetch)
    assert all(_bits(a) == _bits(b) for a, b in zip(got, base))
    # the build alone: the grid's cell_begin and the set of (point, index) rows are those of a grid built in plain order (the order inside a cell is not defined)
    rows = lambda g: (g.cell_begin.cpu().numpy(), np.sort(g.sorted.cpu().numpy().view(np.int64).reshape(-1, 2), axis=0), g.blob[:g.plan.planes_at + 6 * g.plan.res].cpu().numpy())
    plain = run_plain(torch, [sy], lambda: psdr.PointGrid(sy.buf), rows)
    got = run_on_stream(torch, S, form, [sy], lambda: psdr.PointGrid(sy.buf), rows)
    assert all(_bits(a) == _bits(b) for a, b in zip(got, plain))
    # the search: of a grid built in the call, and of one built before on the default stream
    got = run_on_stream(torch, S, form, [sx, sy], lambda: psdr.nearest_points(sx.buf, sy.buf, search="grid", return_stats=True), fetch)
    assert _bits(got[0]) == _bits(base[4]) and _bits(got[1]) == _bits(base[5]) and got[2][0] == 0 and got[2][1] > 0
    grid = psdr.PointGrid(torch.from_numpy(y).cuda())
    torch.cuda.synchronize()
    got = run_on_stream(torch, S, form, [sx], lambda: psdr.nearest_points(sx.buf, grid), fetch)
    assert _bits(got[0]) == _bits(base[4]) and _bits(got[1]) == _bits(base[5])


def test_autograd_reaches_the_mesh_through_the_sampler(psdr):
    import torch
    v, f = cref.bunny()
    target = torch.from_numpy((v + 0.05 * np.sin(3.0 * v[:, [1, 2, 0]])).astype(np.float32)).cuda()
    sam = psdr.SurfaceSampler(f, len(v), num_points=3000, seed=2).resample(v)
    grid = psdr.PointGrid(target)
    grads = []
    for cd, kw in ((psdr.ChamferDistance(), {}), (psdr.ChamferDistance(search="grid"), {}), (psdr.ChamferDistance(search="grid"), dict(y_grid=grid))):
        leaf = torch.from_numpy(v).cuda().requires_grad_()
        loss = cd(sam(leaf), target, **kw)
        loss.backward()
        assert leaf.grad is not None and leaf.grad.shape == leaf.shape and bool(leaf.grad.abs().sum() > 0)
        grads.append((_bits(loss.detach().cpu().numpy()), _bits(leaf.grad.cpu().numpy())))
    assert grads[1] == grads[0] and grads[2] == grads[0]
