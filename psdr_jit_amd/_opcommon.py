"""What the stand-alone operator modules share, stated once: the argument checks that several of them apply, the one-GPU guard, the host-side vertex index and the
device-side inverted index, and the split of a scan into query blocks x candidate slices (csrc/hip/nn_scan.h: plan_of states it in C).  Private: the operator modules
import from here, not from each other.  Torch stays a lazy import."""
import numpy as _np

MAX_COUNT = 1 << 26          # points, vertices, faces of one call
MAX_LATTICE = 1 << 24        # vertices of a lattice
SCAN_THREADS = 256           # lanes of a scan's workgroup
NARROW_MAX = 1024            # more queries than this: the wide scan, several queries per lane
TARGET_GROUPS = 2048         # workgroups a scan's grid aims at: 8 per CU


def _ceil_div(a, b):
    return -(-a // b)


def _single_gpu(what):
    from . import _shard
    if _shard()[1] > 1:
        raise RuntimeError("%s: the denoiser runs on one GPU, torch.distributed is initialised with %d ranks" % (what, _shard()[1]))


def _as_tensor(a):
    import torch
    return a if isinstance(a, torch.Tensor) else torch.as_tensor(_np.asarray(a))


def _checked_shape(shape, what):
    try:
        s = tuple(shape)
    except TypeError:
        raise ValueError("%s: shape must be three integers (nx, ny, nz), got %r" % (what, shape)) from None
    if len(s) != 3 or any(isinstance(n, bool) or not isinstance(n, (int, _np.integer)) for n in s):
        raise ValueError("%s: shape must be three integers (nx, ny, nz), got %r" % (what, shape))
    s = tuple(int(n) for n in s)
    if min(s) < 2:
        raise ValueError("%s: shape = %r, every extent must be at least 2" % (what, s))
    if s[0] * s[1] * s[2] > MAX_LATTICE:
        raise ValueError("%s: shape = %r has %d lattice vertices, at most 2^24" % (what, s, s[0] * s[1] * s[2]))
    return s


def _checked_points(p, what, name):
    p = _as_tensor(p)
    if p.dim() != 2 or p.shape[1] != 3 or p.shape[0] < 1:
        raise ValueError("%s: %s must be [N, 3] with N >= 1, got shape %s" % (what, name, tuple(p.shape)))
    if not p.is_floating_point():
        raise ValueError("%s: %s must be a floating-point tensor, got %s" % (what, name, p.dtype))
    if p.shape[0] > MAX_COUNT:
        raise ValueError("%s: %s has %d points, at most 2^26" % (what, name, p.shape[0]))
    return p


def _faces_checked(faces, n, what):
    f = _np.asarray(faces)
    if f.size == 0:
        f = _np.zeros((0, 3), dtype=_np.int64)
    if f.ndim != 2 or f.shape[1] != 3:
        raise ValueError("%s: faces must be [f, 3], got shape %s" % (what, tuple(f.shape)))
    if not _np.issubdtype(f.dtype, _np.integer):
        raise ValueError("%s: faces must hold integer ids" % what)
    f = f.astype(_np.int64)
    if n <= 0:
        raise ValueError("%s: the number of vertices must be positive" % what)
    if n > MAX_COUNT:
        raise ValueError("%s: %d vertices, at most 2^26" % (what, n))
    if f.size and (f.min() < 0 or f.max() >= n):
        raise ValueError("%s: an id is outside [0, %d)" % (what, n))
    bad = _np.nonzero((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 2] == f[:, 0]))[0]
    if bad.size:
        raise ValueError("%s: face %d repeats a vertex id: %s" % (what, int(bad[0]), f[bad[0]].tolist()))
    return f


def _vertex_index(table, n):
    """host-side numpy: per vertex the (element, role) pairs of `table` [count, roles] that name it, in ascending (element, role) order: (begin [n + 1], elem, role)"""
    count, roles = table.shape
    vertex = table.reshape(-1)
    code = _np.arange(count * roles, dtype=_np.int64)              # element * roles + role: ascending in both
    order = _np.argsort(vertex, kind="stable")                     # by vertex; inside a vertex the codes keep their ascending order
    begin = _np.zeros(n + 1, dtype=_np.int64)
    _np.cumsum(_np.bincount(vertex, minlength=n), out=begin[1:])
    code = code[order]
    i32 = _np.int32
    return begin.astype(i32), (code // roles).astype(i32), (code % roles).astype(i32)


def _inverted(index, count):
    """index int32 [K] with values in [0, count) on the device -> (begin int32 [count + 1], list int32 [K]): per value the positions that hold it, ascending (a stable
    sort); no host synchronisation"""
    import torch
    ordered, order = torch.sort(index, stable=True)
    begin = torch.searchsorted(ordered, torch.arange(count + 1, device=index.device, dtype=torch.int32), out_int32=True)
    return begin, order.to(torch.int32)


def slice_plan(n, m, tile, wide, what):
    """How a scan of n queries over m candidates is split: (tile, queries_per_lane, slices, slice_len), a pure function.  tile: candidates per LDS tile; wide: queries per
    lane above NARROW_MAX queries; what: the ValueError's text for counts outside [1, 2^26].

    A workgroup holds 256 queries_per_lane queries; slice s holds the candidates [s slice_len, min(m, (s + 1) slice_len)); the grid is query blocks x slices."""
    if not (1 <= n <= MAX_COUNT and 1 <= m <= MAX_COUNT):
        raise ValueError(what)
    qpl = wide if n > NARROW_MAX else 1
    qblocks = _ceil_div(n, SCAN_THREADS * qpl)
    tiles = _ceil_div(m, tile)
    want = min(_ceil_div(TARGET_GROUPS, qblocks), tiles)
    slice_len = _ceil_div(tiles, want) * tile
    return tile, qpl, _ceil_div(m, slice_len), slice_len
