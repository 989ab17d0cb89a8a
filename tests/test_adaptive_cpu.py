"""Adaptive sampling, what can be checked without a GPU: the entry points are declared, exported and listed and the ABI did not move; every entry point refuses
bad arguments before it touches a device; the allocation rule, restated here with Python integers (`allocate`, which tests/test_gpu_adaptive.py compares the
kernels against bit for bit), has the invariants the rule promises; the elementwise Python pieces follow their formulas."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("psdr_hip_adaptive_scratch_bytes", "psdr_hip_adaptive_bits", "psdr_hip_adaptive_counts", "psdr_hip_adaptive_expand", "psdr_hip_adaptive_merge",
       "psdr_hip_adaptive_merge_adj")
N_MAX = 1 << 24


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement of psdr_hip_adaptive_counts (include/psdr_hip.h)
def ceil_log2(v):
    """the smallest b with 2^b >= v, v >= 1"""
    return (int(v) - 1).bit_length()


def bits_for(n, budget):
    return min(20, 62 - ceil_log2(n) - ceil_log2(max(int(budget), 1)))


def quantise(weights, bits):
    """(q as Python integers in an object array, the cleaned float32 weights)"""
    w = np.asarray(weights, dtype=np.float32).reshape(-1)
    with np.errstate(invalid="ignore"):
        w = np.where(np.isfinite(w) & (w > 0), w, np.float32(0)).astype(np.float32)
    wmax = w.max()
    if wmax > 0:
        q = np.floor(w.astype(np.float64) / np.float64(wmax) * float(2 ** bits)).astype(np.uint32)       # two correctly rounded float64 operations, as on the device
    else:
        q = np.ones(w.size, dtype=np.uint32)
    return q.astype(object), w


def allocate(weights, budget, min_count=0):
    """counts [n], offsets [n + 1] (int64 arrays), q (object array) and S of the allocation rule; every product and quotient in Python integers"""
    n = int(np.asarray(weights).size)
    budget, min_count = int(budget), int(min_count)
    bits = bits_for(n, budget)
    assert 0 < n <= N_MAX and bits >= 8 and 0 <= n * min_count <= budget <= 2 ** 31 - 1
    q, _ = quantise(weights, bits)
    if int(q.sum()) == 0:
        q = np.ones(n, dtype=np.uint32).astype(object)
    prefix = np.empty(n + 1, dtype=object)
    prefix[0] = 0
    prefix[1:] = np.cumsum(q)
    S = int(prefix[n])
    assert (budget - n * min_count) * S < 2 ** 62
    floors = ((budget - n * min_count) * prefix) // S
    counts = min_count + (floors[1:] - floors[:-1])
    offsets = np.arange(n + 1, dtype=object) * min_count + floors
    return counts.astype(np.int64), offsets.astype(np.int64), q, S


def weight_maps(n, rng):
    """the maps both test files use"""
    hot = np.zeros(n, dtype=np.float32)
    hot[(7 * n) // 11] = 3.5
    bad = rng.random(n).astype(np.float32)
    bad[::3] = np.nan
    bad[1::5] = np.inf
    bad[2::7] = -1.0
    bad[n // 2] = 0.25                                       # (n = 1: the only pixel is finite again)
    return {"random": rng.random(n).astype(np.float32), "hot": hot, "bad": bad, "zero": np.zeros(n, dtype=np.float32),
            "wide": (10.0 ** rng.uniform(-15.0, 15.0, n)).astype(np.float32)}


def budgets(n, min_count):
    return sorted({b for b in (0, 1, n - 1, 7 * n + 3) if b >= n * min_count})


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def psdr():
    import __graft_entry__
    __graft_entry__.build()
    import psdr_jit_amd
    return psdr_jit_amd


def test_entry_points_declared_exported_listed(psdr):
    from psdr_jit_amd import cabi
    with open(os.path.join(ROOT, "include", "psdr_hip.h")) as fh:
        text = fh.read()
    L = cabi.lib()
    for name in NEW:
        assert re.search(r"^(int|int64_t)\s+%s\s*\(" % name, text, re.M), "%s is not declared in include/psdr_hip.h" % name
        assert hasattr(L, name), "libpsdr_hip.so does not export %s" % name
        assert name in cabi.SYMBOLS
        assert getattr(L, name).argtypes is not None, "%s has no argtypes" % name
    assert re.search(r"#define\s+PSDR_HIP_ABI_VERSION\s+16\b", text)
    assert L.psdr_hip_abi_version() == 16
    assert C.sizeof(cabi.RenderArgs) == 128
    for name in ("adaptive_weights", "PixelPlan", "render_c_adaptive"):
        assert hasattr(psdr, name)
    assert int(L.psdr_hip_adaptive_scratch_bytes()) >= 16 + 12 * (N_MAX // 2048)
    for n, budget in ((1, 0), (1, 1), (2, 2), (3, 5), (512 * 512, 512 * 512 * 32), (N_MAX, 2 ** 30), (N_MAX, 2 ** 30 + 1), (N_MAX, 2 ** 31 - 1), (1025, 7 * 1025 + 3)):
        assert L.psdr_hip_adaptive_bits(n, budget) == bits_for(n, budget), (n, budget)
    assert bits_for(N_MAX, 2 ** 30) == 8 and bits_for(N_MAX, 2 ** 30 + 1) == 7 and bits_for(512 * 512, 512 * 512 * 32) == 20


def test_every_entry_point_refuses_bad_arguments_before_any_device_call(psdr):
    """no GPU is visible here: a call that reached the device would fail with a HIP error, not with the entry point's own message.  The non-NULL pointers are host
    addresses that a refused call never reads."""
    from psdr_jit_amd import cabi
    L = cabi.lib()
    host = np.zeros(64, dtype=np.int64)
    p = host.ctypes.data

    def refused(rc, name, word):
        msg = L.psdr_hip_last_error().decode()
        assert rc != 0 and msg.startswith(name + ":") and word in msg and "hip" not in msg[len(name):].lower(), (name, word, rc, msg)

    name = "psdr_hip_adaptive_counts"
    for k in (0, 4, 5, 6):
        args = [p, 16, 32, 0, p, p, p, None]
        args[k] = None
        refused(L.psdr_hip_adaptive_counts(*args), name, "NULL")
    refused(L.psdr_hip_adaptive_counts(p, 0, 32, 0, p, p, p, None), name, "n = 0")
    refused(L.psdr_hip_adaptive_counts(p, -5, 32, 0, p, p, p, None), name, "n = -5")
    refused(L.psdr_hip_adaptive_counts(p, N_MAX + 1, 32, 0, p, p, p, None), name, "2^24")
    refused(L.psdr_hip_adaptive_counts(p, 16, -1, 0, p, p, p, None), name, "negative")
    refused(L.psdr_hip_adaptive_counts(p, 16, 31, 2, p, p, p, None), name, "n * min_count")
    refused(L.psdr_hip_adaptive_counts(p, 16, 32, -1, p, p, p, None), name, "min_count")
    refused(L.psdr_hip_adaptive_counts(p, 16, 2 ** 31, 0, p, p, p, None), name, "2^31 - 1")
    refused(L.psdr_hip_adaptive_counts(p, N_MAX, 2 ** 31 - 1, 0, p, p, p, None), name, "fewer than 8")
    refused(L.psdr_hip_adaptive_counts(p, N_MAX, 2 ** 30 + 1, 0, p, p, p, None), name, "fewer than 8")

    name = "psdr_hip_adaptive_expand"
    refused(L.psdr_hip_adaptive_expand(None, 16, 32, p, None), name, "NULL")
    refused(L.psdr_hip_adaptive_expand(p, 16, 32, None, None), name, "NULL")
    refused(L.psdr_hip_adaptive_expand(p, 0, 32, p, None), name, "n = 0")
    refused(L.psdr_hip_adaptive_expand(p, 16, -1, p, None), name, "total")
    refused(L.psdr_hip_adaptive_expand(p, 16, 2 ** 31, p, None), name, "total")
    assert L.psdr_hip_adaptive_expand(p, 16, 0, None, None) == 0                   # an empty list: nothing to do, and no launch

    name = "psdr_hip_adaptive_merge"
    good = [p, 16, 32, 3, p, 4.0, p, 4.0, 0, p, None]

    def merge_with(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return L.psdr_hip_adaptive_merge(*a)
    refused(merge_with(a0=None), name, "NULL")
    refused(merge_with(a4=None), name, "NULL")
    refused(merge_with(a9=None), name, "NULL")
    refused(merge_with(a6=None), name, "base is NULL")
    refused(merge_with(a1=0), name, "n must be positive")
    refused(merge_with(a2=-1), name, "total")
    refused(merge_with(a3=0), name, "channels")
    refused(merge_with(a3=5), name, "channels")
    refused(merge_with(a5=0.0), name, "rows_n")
    refused(merge_with(a5=float("nan")), name, "rows_n")
    refused(merge_with(a7=-1.0), name, "base_n")
    refused(merge_with(a8=2), name, "square")

    name = "psdr_hip_adaptive_merge_adj"
    good_adj = [p, 16, 32, 3, p, 4.0, 4.0, p, p, None]
    for k, word in ((0, "NULL"), (4, "NULL"), (7, "NULL")):
        a = list(good_adj)
        a[k] = None
        refused(L.psdr_hip_adaptive_merge_adj(*a), name, word)
    for k, v, word in ((1, -2, "n must be positive"), (2, 2 ** 31, "total"), (3, 7, "channels"), (5, -1.0, "rows_n"), (6, float("inf"), "base_n")):
        a = list(good_adj)
        a[k] = v
        refused(L.psdr_hip_adaptive_merge_adj(*a), name, word)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1025, 5000])
def test_the_rule_keeps_its_promises(n):
    rng = np.random.default_rng(100 + n)
    for label, w in weight_maps(n, rng).items():
        for min_count in (0, 2):
            for budget in budgets(n, min_count) + [11 * n]:
                counts, offsets, q, S = allocate(w, budget, min_count)
                spare = budget - n * min_count
                assert int(counts.sum()) == budget and counts.min() >= min_count, (label, n, budget, min_count)
                assert offsets[0] == 0 and offsets[n] == budget and np.array_equal(np.diff(offsets), counts)
                # within one of the ideal share, in integers: |(counts_i - min_count) S - B' q_i| < S
                for c, qi in zip(counts.tolist(), q.tolist()):
                    assert abs((c - min_count) * S - spare * qi) < S, (label, n, budget, min_count, c, qi)
    # a pixel without weight gets min_count and nothing more; the hot pixel gets all the rest
    counts, _, _, _ = allocate(weight_maps(n, rng)["hot"], 7 * n + 3, 2)
    if n > 1:
        assert sorted(set(counts.tolist())) == [2, 2 + 5 * n + 3] and counts[(7 * n) // 11] == 2 + 5 * n + 3


def test_uniform_allocations():
    rng = np.random.default_rng(5)
    for n in (1, 7, 64, 1000):
        for k in (0, 1, 5):
            for w in (np.full(n, 0.37, np.float32), np.zeros(n, np.float32), np.full(n, np.nan, np.float32), -rng.random(n).astype(np.float32),
                      np.full(n, np.inf, np.float32)):
                counts, offsets, _, _ = allocate(w, k * n)
                assert np.array_equal(counts, np.full(n, k)) and np.array_equal(offsets, k * np.arange(n + 1))
        # no weight anywhere and a budget that does not divide: the counts differ by at most one
        counts, _, _, _ = allocate(np.zeros(n, np.float32), 3 * n + n // 2)
        assert counts.max() - counts.min() <= 1 and counts.sum() == 3 * n + n // 2


def test_python_pieces_follow_their_formulas(psdr, monkeypatch):
    import torch
    rng = np.random.default_rng(9)
    n_pix, spp = 40, 8
    x = rng.random((n_pix, spp, 3)) * np.array([1.0, 0.5, 2.0])
    x[3] = 0.0                                                # a black pixel
    mean, sq = x.mean(axis=1), ((x / spp) ** 2).sum(axis=1)
    sigma = np.sqrt(x.var(axis=1, ddof=1).sum(axis=1))        # the per-sample standard deviation, channels added in variance
    w = psdr.adaptive_weights(torch.from_numpy(mean), torch.from_numpy(sq), spp).numpy()
    assert w.shape == (n_pix,) and np.abs(w - sigma).max() <= 1e-9 and w[3] == 0.0
    wr = psdr.adaptive_weights(torch.from_numpy(mean), torch.from_numpy(sq), spp, mode="relative", eps=0.5).numpy()
    assert np.abs(wr - sigma / (mean.sum(axis=1) + 0.5)).max() <= 1e-9
    with pytest.raises(ValueError, match="mode"):
        psdr.adaptive_weights(torch.from_numpy(mean), torch.from_numpy(sq), spp, mode="other")
    with pytest.raises(ValueError):
        psdr.adaptive_weights(torch.from_numpy(mean), torch.from_numpy(sq), 1)
    # samples and variance with a per-pixel n (host tensors: nothing here needs the device)
    counts = torch.tensor([0, 1, 3, 0], dtype=torch.int32)
    offsets = torch.tensor([0, 0, 1, 4, 4], dtype=torch.int32)
    plan = psdr.PixelPlan(counts, offsets, torch.tensor([1, 2, 2, 2], dtype=torch.int32), 4, 4)
    assert plan.samples(2.0, 1.0).tolist() == [1.0, 3.0, 7.0, 1.0] and plan.samples(4).tolist() == [0.0, 4.0, 12.0, 0.0]
    img = torch.tensor(rng.random((4, 3)))
    sq4 = img * img * 0.6
    var = plan.variance(img, sq4, 2.0, 1.0).numpy()
    nn = np.array([1.0, 3.0, 7.0, 1.0])[:, None]
    want = np.where(nn > 1, (sq4.numpy() - img.numpy() ** 2 / np.maximum(nn, 2)) * (np.maximum(nn, 2) / (np.maximum(nn, 2) - 1)), 0.0)
    assert np.array_equal(var[[0, 3]], np.zeros((2, 3))) and np.abs(var - want).max() <= 1e-15
    # one GPU only: a clear error before anything is launched
    monkeypatch.setattr(psdr, "_shard", lambda: (0, 2))
    with pytest.raises(RuntimeError, match="one GPU"):
        psdr.PixelPlan.from_weights(torch.ones(8), 16)
    with pytest.raises(RuntimeError, match="one GPU"):
        psdr.render_c_adaptive(None, None, 16, seed=1)
    with pytest.raises(RuntimeError, match="one GPU"):
        plan.merge(torch.zeros((4, 3)), 2.0)
