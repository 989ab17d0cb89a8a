"""Exact nearest neighbours through a uniform grid over the candidates (kernels: csrc/hip/nn_grid.h, entry points in csrc/hip/chamfer.hip).

The scan of chamfer.py tests every (query, candidate) pair; for clouds of 10^5 points and more that is the whole cost of a shape term.  The grid returns THE SAME two
arrays, bit for bit - the lowest index of the minimum of the float32 d2 of chamfer.py's definition - after testing only the candidates near a query:

    grid = psdr.PointGrid(target_points)                                # once, while target_points does not change
    index, dist2 = psdr.nearest_points(x, grid)                         # or psdr.nearest_points(x, y, search="grid"), which builds the grid of y first
    cd = psdr.ChamferDistance(search="grid");  loss = cd(sam(v), target_points, y_grid=grid)

How (include/psdr_hip.h states it in full).  The candidates are sorted into res^3 cells of their bounding box, res a function of m alone (grid_plan).  A query visits
the cells round its own shell by shell and stops as soon as a float32 bound proves that no unvisited cell holds a candidate that beats or ties its best; a query that
cannot stop within max_shells shells (far outside the box, in the hollow of a surface cloud, between two clusters) is finished exactly by a brute-force pass.  Nothing is
read back to the host: the build and the search are plain launches on torch's current stream.

grid_plan(n, m) is the plan that psdr_hip_chamfer_grid_plan states in C, a pure function.  The default search everywhere stays "scan"; there is no "auto"."""
import collections as _collections

from ._opcommon import MAX_COUNT, _ceil_div, _checked_points, _single_gpu

PER_CELL = 2                 # candidates per cell the resolution aims at: res = the largest r with PER_CELL r^3 <= m
MAX_RES = 256                # cells per axis at most
MIN_SHELLS, MAX_SHELLS = 4, 16   # the shell budget is res // 4 within these bounds; a query not certified within it goes to the fallback
HEADER = 16                  # 32-bit words ahead of the planes
SCAN_CHUNK = 2048            # cells per workgroup of the exclusive scan
TILE = 1024                  # candidates per LDS tile of the fallback
FALLBACK_GROUPS = 64         # the fallback's fixed grid: query-block striders x candidate slices
FALLBACK_SLICES = 32
GROUP_LANES, GROUP_MAX = 8, 65536   # lanes per query of the walk up to GROUP_MAX queries (8 x 65 536 lanes fill the device), one lane per query beyond
WORK_HEAD = 8                # 32-bit words ahead of the build's per-candidate work arrays
SEARCHES = ("scan", "grid")

GridPlan = _collections.namedtuple("GridPlan", [
    "res", "max_shells",                       # cells per axis; shells a query may visit before the fallback takes it
    "cells",                                    # entries of cell_begin: res^3 + 1
    "planes_at", "begin_at", "points_at",       # where the planes [6 res], cell_begin [cells] and the sorted candidates [4 m] start in the grid blob, in 32-bit words
    "grid_words", "work_words",                 # lengths of the grid blob and of the build's work array, in 32-bit words
    "keys_len", "list_len", "stats_len",        # lengths of the search's arrays: keys uint64 [n], list int32 [n], stats uint64 [2]
    "fallback_groups", "fallback_slices", "fallback_slice_len",
    "lanes_per_query",                          # lanes that share one query's walk: a function of n
])


def grid_plan(n, m):
    """The grid of m candidates and the work arrays of a search of n queries in it: a GridPlan, a pure function (csrc/hip/nn_grid.h: grid_plan_of).

    res = the largest r in [1, 256] with 2 r^3 <= m (1 for m < 16): two candidates per cell of a full box, several per occupied cell of a surface cloud; a function of m
    alone.  max_shells = res // 4 within [4, 16]: a query walks a quarter of the box at most (at 16 shells some 7 000 cell ranges, far below the m of such a grid) before
    the fallback scans all m candidates for it.  The grid blob holds a header of 16 words, the 6 res planes of the stopping rule, cell_begin and the candidates in cell order as (x, y, z, index), the last two
    aligned to 4 words.  The fallback scans with a fixed grid of fallback_groups x fallback_slices workgroups, slice s holding the candidates
    [s fallback_slice_len, min(m, (s + 1) fallback_slice_len)).  lanes_per_query lanes share a query's walk: 8 up to 65 536 queries, 1 beyond; the results and the
    statistics do not depend on it."""
    n, m = int(n), int(m)
    if not (1 <= n <= MAX_COUNT and 1 <= m <= MAX_COUNT):
        raise ValueError("grid_plan: n = %d, m = %d, both must lie in [1, 2^26]" % (n, m))
    r = 1
    while r < MAX_RES and PER_CELL * (r + 1) ** 3 <= m:
        r += 1
    cells = r ** 3 + 1
    planes_at = HEADER
    begin_at = _ceil_div(planes_at + 6 * r, 4) * 4
    points_at = _ceil_div(begin_at + cells, 4) * 4
    scan_groups = _ceil_div(cells, SCAN_CHUNK)
    tiles = _ceil_div(m, TILE)
    slice_len = _ceil_div(tiles, min(tiles, FALLBACK_SLICES)) * TILE
    return GridPlan(r, min(MAX_SHELLS, max(MIN_SHELLS, r // 4)), cells, planes_at, begin_at, points_at, points_at + 4 * m, WORK_HEAD + 2 * m + scan_groups, n, n, 2,
                    FALLBACK_GROUPS, _ceil_div(m, slice_len), slice_len, GROUP_LANES if n <= GROUP_MAX else 1)


def _checked_search(search, what):
    if search not in SEARCHES:
        raise ValueError("%s: search must be one of %s, got %r" % (what, ", ".join(repr(s) for s in SEARCHES), search))
    return search


class PointGrid:
    """The uniform grid of a candidate set y [M, 3]: built on torch's current stream without a host synchronisation, reusable while y does not change.

    It holds device tensors only: `points` (y as float32 on the render device, which the fallback scans), and `blob`, the int32 array psdr_hip_chamfer_grid_build fills,
    of which box (lo[3], inv[3], width[3] as float32), dims (cells per axis: res, or 1 for an axis of zero extent), planes [6 res], cell_begin [res^3 + 1] and sorted
    [M, 4] (x, y, z and the bits of the original index, in cell order) are views.  plan: grid_plan(1, M).  Work queued on another stream must wait for the stream the grid
    was built on, as for any tensor."""

    def __init__(self, y):
        y = _checked_points(y, "PointGrid", "y")
        _single_gpu("PointGrid")
        import torch
        from . import cabi, _device, _stream_ptr
        device = _device()
        self.points = y.detach().to(device, torch.float32).contiguous()
        self.num_points = m = int(self.points.shape[0])
        self.plan = p = grid_plan(1, m)
        with torch.cuda.device(device):
            self.blob = torch.empty(p.grid_words, device=device, dtype=torch.int32)
            work = torch.empty(p.work_words, device=device, dtype=torch.int32)
            cabi.check(cabi.lib().psdr_hip_chamfer_grid_build(self.points.data_ptr(), m, self.blob.data_ptr(), p.grid_words, work.data_ptr(), p.work_words, _stream_ptr()))
        self.box = self.blob[0:9].view(torch.float32)
        self.dims = self.blob[9:12]
        self.planes = self.blob[p.planes_at:p.planes_at + 6 * p.res].view(torch.float32)
        self.cell_begin = self.blob[p.begin_at:p.begin_at + p.cells]
        self.sorted = self.blob[p.points_at:p.points_at + 4 * m].view(m, 4)

    @property
    def device(self):
        return self.points.device


def _checked_grid(grid, what, name):
    """a PointGrid on the render device, checked without looking for a device when it is wrong"""
    import torch
    if not isinstance(grid, PointGrid):
        raise ValueError("%s: %s must be a PointGrid, got %s" % (what, name, type(grid).__name__))
    tensors = (grid.points, grid.blob)
    if grid.points.dtype != torch.float32 or grid.blob.dtype != torch.int32 or grid.points.dim() != 2 or grid.points.shape[1] != 3:
        raise ValueError("%s: %s holds points of dtype %s and a blob of dtype %s, expected float32 [M, 3] and int32" % (what, name, grid.points.dtype, grid.blob.dtype))
    if not all(t.is_cuda for t in tensors) or grid.points.device != grid.blob.device:
        raise ValueError("%s: %s lies on %s, not on a GPU" % (what, name, grid.points.device))
    p = grid_plan(1, int(grid.points.shape[0]))
    if int(grid.blob.numel()) < p.grid_words or not grid.blob.is_contiguous() or not grid.points.is_contiguous():
        raise ValueError("%s: %s has a blob of %d words, its %d points need %d" % (what, name, grid.blob.numel(), grid.points.shape[0], p.grid_words))
    return grid


def _on_render_device(grid, device, what, name):
    if grid.points.device != device:
        raise ValueError("%s: %s lies on %s, the render device is %s" % (what, name, grid.points.device, device))


def _grid_nearest(x, grid, device, want_stats=False):
    """x: float32 contiguous on `device`; grid: a checked PointGrid there -> (index int32 [N], dist2 float32 [N], stats int64 [2] or None) on the current stream"""
    import torch
    from . import cabi, _stream_ptr
    n, m = int(x.shape[0]), grid.num_points
    p = grid_plan(n, m)
    keys = torch.empty(p.keys_len, device=device, dtype=torch.int64)
    work = torch.empty(p.list_len, device=device, dtype=torch.int32)
    stats = torch.empty(p.stats_len, device=device, dtype=torch.int64)
    index = torch.empty(n, device=device, dtype=torch.int32)
    dist2 = torch.empty(n, device=device, dtype=torch.float32)
    cabi.check(cabi.lib().psdr_hip_chamfer_grid_nearest(x.data_ptr(), n, grid.points.data_ptr(), m, grid.blob.data_ptr(), p.grid_words, keys.data_ptr(), work.data_ptr(),
                                                        index.data_ptr(), dist2.data_ptr(), stats.data_ptr(), _stream_ptr()))
    return index, dist2, (stats if want_stats else None)
