"""The variance-guided a-trous denoiser, what can be checked without a GPU: the entry points are declared, exported and listed and the ABI did not move; every entry point
refuses bad arguments before it touches a device; the float64 restatement (tests/vdenoise_ref.py, which tests/test_gpu_vdenoise.py compares the kernels against) has the
properties the specification promises, and on the step frames of the issue it gives the figures the issue states; the Python surface refuses wrong arguments."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import denoise_ref as dref
import test_denoise_cpu as dcpu
import vdenoise_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("psdr_hip_vdenoise_create", "psdr_hip_vdenoise_apply", "psdr_hip_vdenoise_frozen", "psdr_hip_vdenoise_frozen_adj", "psdr_hip_vdenoise_record",
       "psdr_hip_vdenoise_destroy")
EPS = 1e-12


@pytest.fixture(scope="module")
def psdr():
    import __graft_entry__
    __graft_entry__.build()
    import psdr_jit_amd
    return psdr_jit_amd


def test_entry_points_declared_exported_listed(psdr):
    from psdr_jit_amd import build, cabi
    with open(os.path.join(ROOT, "include", "psdr_hip.h")) as fh:
        text = fh.read()
    L = cabi.lib()
    for name in NEW:
        assert re.search(r"^int\s+%s\s*\(" % name, text, re.M), "%s is not declared in include/psdr_hip.h" % name
        assert hasattr(L, name), "libpsdr_hip.so does not export %s" % name
        assert name in cabi.SYMBOLS
        assert getattr(L, name).argtypes is not None, "%s has no argtypes" % name
    assert re.search(r"#define\s+PSDR_HIP_ABI_VERSION\s+16\b", text)
    assert L.psdr_hip_abi_version() == 16
    for name in ("VarianceDenoiser", "luminance_variance"):
        assert hasattr(psdr, name)
    units = {u[0]: u for u in build.hip_units()}
    assert units["vdenoise"][1].endswith("vdenoise.hip")
    deps = {os.path.relpath(d, ROOT) for d in units["vdenoise"][3]}
    assert {os.path.join("include", "psdr_hip.h"), os.path.join("psdr_jit_amd", "csrc", "hip", "atrous.h"), os.path.join("psdr_jit_amd", "isa_lint.py")} <= deps


def test_every_entry_point_refuses_bad_arguments_before_any_device_call(psdr):
    """no GPU is visible here: a call that reached the device would fail with a HIP error, not with the entry point's own message.  The non-NULL device pointers are host
    addresses that a refused call never reads; a frozen call without a record can only be shown on a real handle, which tests/test_gpu_vdenoise.py does."""
    from psdr_jit_amd import cabi
    L = cabi.lib()
    host = np.zeros(64, dtype=np.int64)
    p, p2, p3, p4 = (host.ctypes.data + 64 * i for i in range(4))
    a3 = (C.c_float * 3)(0.2126, 0.7152, 0.0722)

    def refused(rc, name, word):
        msg = L.psdr_hip_last_error().decode()
        assert rc != 0 and msg.startswith(name + ":") and word in msg and "hip" not in msg[len(name):].lower(), (name, word, rc, msg)

    name = "psdr_hip_vdenoise_create"
    h = C.c_void_p()
    refused(L.psdr_hip_vdenoise_create(p, 3, 16, 16, 5, None, None), name, "NULL")
    refused(L.psdr_hip_vdenoise_create(None, 3, 16, 16, 5, C.byref(h), None), name, "NULL")
    for W, H, word in ((0, 16, "W = 0"), (16, 0, "H = 0"), (-3, 16, "W = -3"), (16, -1, "H = -1"), (4097, 4096, "2^24"), (1 << 24, 2, "2^24"), (1 << 30, 1 << 30, "2^24")):
        refused(L.psdr_hip_vdenoise_create(p, 3, W, H, 5, C.byref(h), None), name, word)
    for Lv in (0, -1, 9):
        refused(L.psdr_hip_vdenoise_create(p, 3, 16, 16, Lv, C.byref(h), None), name, "L = %d" % Lv)
    for G in (-1, 9):
        refused(L.psdr_hip_vdenoise_create(p, G, 16, 16, 5, C.byref(h), None), name, "G = %d" % G)
    assert not h.value                                        # a refused create leaves no handle behind

    fake = C.c_void_p(p)                                      # (a refused call never looks into the handle)
    name = "psdr_hip_vdenoise_apply"
    fn = L.psdr_hip_vdenoise_apply
    refused(fn(None, p, 3, p2, a3, 0.25, EPS, p3, p4, None), name, "NULL")
    refused(fn(fake, None, 3, p2, a3, 0.25, EPS, p3, p4, None), name, "NULL")
    refused(fn(fake, p, 3, None, a3, 0.25, EPS, p3, p4, None), name, "NULL")
    refused(fn(fake, p, 3, p2, None, 0.25, EPS, p3, p4, None), name, "NULL")
    refused(fn(fake, p, 3, p2, a3, 0.25, EPS, None, p4, None), name, "NULL")
    for Cv in (0, 2, 4, -1):
        refused(fn(fake, p, Cv, p2, a3, 0.25, EPS, p3, p4, None), name, "C must")
    refused(fn(fake, p, 3, p2, a3, 0.25, EPS, p, p4, None), name, "in and out")
    refused(fn(fake, p, 3, p2, a3, 0.25, EPS, p3, p2, None), name, "var and var_out")
    for k in (-1.0, float("nan"), float("inf")):
        refused(fn(fake, p, 3, p2, a3, k, EPS, p3, p4, None), name, "k = ")
    for eps in (0.0, -1e-12, float("nan"), float("inf")):
        refused(fn(fake, p, 3, p2, a3, 0.25, eps, p3, p4, None), name, "eps = ")
    refused(fn(fake, p, 3, p2, (C.c_float * 3)(0.2, float("nan"), 0.1), 0.25, EPS, p3, p4, None), name, "lum[1]")
    refused(fn(fake, p, 1, p2, (C.c_float * 1)(float("inf")), 0.25, EPS, p3, p4, None), name, "lum[0]")
    for name in ("psdr_hip_vdenoise_frozen", "psdr_hip_vdenoise_frozen_adj"):
        fn = getattr(L, name)
        refused(fn(None, p, 3, p2, None), name, "NULL")
        refused(fn(fake, None, 3, p2, None), name, "NULL")
        refused(fn(fake, p, 3, None, None), name, "NULL")
        for Cv in (0, 2, 4):
            refused(fn(fake, p, Cv, p2, None), name, "C must")
        refused(fn(fake, p, 3, p, None), name, "different")
        blank = np.zeros(64, dtype=np.int64)                 # a handle-sized block of zeros: recorded == false
        refused(fn(C.c_void_p(blank.ctypes.data), p, 3, p2, None), name, "no record")
    refused(L.psdr_hip_vdenoise_record(None, p, None), "psdr_hip_vdenoise_record", "NULL")
    refused(L.psdr_hip_vdenoise_record(fake, None, None), "psdr_hip_vdenoise_record", "NULL")
    refused(L.psdr_hip_vdenoise_record(fake, p, None), "psdr_hip_vdenoise_record", "no record")
    refused(L.psdr_hip_vdenoise_destroy(None), "psdr_hip_vdenoise_destroy", "NULL")


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement's own properties, in float64
def _inputs(rng, W, H, C):
    """(x float32 [W H, C], v float32 [W H]): both signs over two decades, v over three decades; where the frame is large enough one block has v = 0 and constant x,
    another v = 0 and varying x"""
    x = (rng.standard_normal((H, W, C)) * 10.0 ** rng.uniform(-1, 1, (H, W, 1))).astype(np.float32)
    v = (10.0 ** rng.uniform(-3, 0, (H, W))).astype(np.float32)
    if W >= 8 and H >= 6:
        x[1:H // 2, 1:W // 3] = np.float32(0.75)
        v[1:H // 2, 1:W // 3] = 0.0
        v[H // 2:, W // 2:W // 2 + W // 4] = 0.0
    return x.reshape(W * H, C), v.reshape(W * H)


def _dense(g, record, k, W, H, l):
    """(A_l, the matrix of w_l) as dense [n, n] matrices from a record"""
    w, N = ref.level_weights(g, record, k, EPS, W, H, l)
    n, s = W * H, 1 << l
    Wm = np.zeros((n, n))
    for t, (i, j) in enumerate(dref.TAPS):
        for y in range(H):
            for x in range(W):
                qx, qy = x + s * i, y + s * j
                if 0 <= qx < W and 0 <= qy < H:
                    Wm[y * W + x, qy * W + qx] += w[t][y, x]
                else:
                    assert w[t][y, x] == 0.0          # a tap outside the frame is dropped
    return Wm * record[l][2].reshape(n, 1), Wm


@pytest.mark.parametrize("W,H,L,G,C", [(33, 9, 5, 8, 3), (67, 35, 3, 1, 1), (5, 3, 3, 0, 1), (9, 7, 4, 2, 3)])
def test_restatement_with_k_0_is_the_denoiser(W, H, L, G, C):
    rng = np.random.default_rng(W + G)
    g = dcpu._guides(rng, W, H, G) if G else None
    x, v = _inputs(rng, W, H, C)
    out, v_out, record = ref.apply(x, v, g, W, H, L, 0.0, EPS)
    assert np.array_equal(out, dref.apply(x, g, W, H, L))
    assert np.isfinite(v_out).all() and (v_out >= 0).all()


@pytest.mark.parametrize("W,H,G,C", [(5, 3, 2, 3), (9, 7, 0, 3), (9, 7, 8, 1)])
def test_restatement_symmetry_matrix_form_and_transpose(W, H, G, C):
    """w_l is symmetric bit for bit; the frozen operator equals the product of its dense matrices, its transpose their transposed product; frozen(x) of the record x made
    is apply(x)"""
    rng = np.random.default_rng(W * 100 + H * 10 + G)
    g = dcpu._guides(rng, W, H, G) if G else None
    x, v = _inputs(rng, W, H, C)
    u = rng.standard_normal((W * H, 3))
    for L in (1, 2, 4):
        out, _, record = ref.apply(x, v, g, W, H, L, 0.25, EPS)
        D = np.eye(W * H)
        for l in range(L):
            A, Wm = _dense(g, record, 0.25, W, H, l)
            assert np.array_equal(Wm, Wm.T)
            assert np.abs(A.sum(axis=1) - 1.0).max() <= 1e-14
            D = A @ D
        assert np.abs(ref.frozen(u, g, record, W, H, 0.25, EPS) - D @ u).max() <= 1e-13 * np.abs(u).max()
        assert np.abs(ref.frozen_adj(u, g, record, W, H, 0.25, EPS) - D.T @ u).max() <= 1e-12 * np.abs(u).max()
        assert np.abs(ref.frozen(x, g, record, W, H, 0.25, EPS) - out).max() <= 1e-13 * np.abs(x).max()
        assert np.abs(D @ x.astype(np.float64) - dref.apply(x, g, W, H, L)).max() > 1e-3          # and it is not the denoiser without the luminance weight


@pytest.mark.parametrize("W,H,L,G,C", [(33, 9, 5, 8, 3), (67, 35, 5, 1, 1), (5, 3, 3, 0, 1), (64, 17, 4, 8, 3)])
def test_restatement_transpose_identity(W, H, L, G, C):
    rng = np.random.default_rng(7 + W)
    g = dcpu._guides(rng, W, H, G) if G else None
    x, v = _inputs(rng, W, H, C)
    record = ref.apply(x, v, g, W, H, L, 0.25, EPS)[2]
    u, y = rng.standard_normal((W * H, 3)), rng.standard_normal((W * H, 3))
    lhs, rhs = (ref.frozen(u, g, record, W, H, 0.25, EPS) * y).sum(), (u * ref.frozen_adj(y, g, record, W, H, 0.25, EPS)).sum()
    assert abs(lhs - rhs) <= 1e-12 * (np.abs(u) * np.abs(y)).sum()


@pytest.mark.parametrize("W,H,G", [(5, 3, 0), (9, 7, 3)])
def test_one_level_of_variance_is_the_diagonal_of_the_covariance(W, H, G):
    """v_1 = diag(A diag(v) A^T): the exact variance of one level's output for independent pixels and fixed weights (C = 1, a = 1: the image is its luminance)"""
    rng = np.random.default_rng(W)
    g = dcpu._guides(rng, W, H, G) if G else None
    x, v = _inputs(rng, W, H, 1)
    _, v1, record = ref.apply(x, v, g, W, H, 1, 0.25, EPS)
    A, _ = _dense(g, record, 0.25, W, H, 0)
    want = np.diag(A @ np.diag(v.astype(np.float64)) @ A.T)
    assert np.abs(v1 - want).max() <= 1e-14 * v.max()


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("what", ["x", "guide", "v"])
@pytest.mark.parametrize("where", ["interior", "corner"])
def test_restatement_non_finite_rule(bad, what, where):
    """A non-finite x or guide at q zeroes exactly the taps that touch q and leaves q's centre tap; a non-finite v at q does so for every pixel of q's 3 x 3 unit
    neighbourhood (vt is non-finite there)."""
    W, H, G = 11, 9, 3
    rng = np.random.default_rng(3)
    g = dcpu._guides(rng, W, H, G) * np.float32(0.1)
    x = (1.0 + 0.1 * rng.standard_normal((W * H, 3))).astype(np.float32)             # (small differences against v: every other weight is well above 0)
    v = np.full(W * H, 0.5, dtype=np.float32)
    k = 0.25
    qx, qy = (5, 4) if where == "interior" else (0, 0)
    q = qy * W + qx
    _, _, clean_rec = ref.apply(x, v, g, W, H, 1, k, EPS)
    clean = ref.level_weights(g, clean_rec, k, EPS, W, H, 0)[0]
    if what == "x":
        x[q, 1] = bad
    elif what == "guide":
        g[q, 1] = bad
    else:
        v[q] = bad
    cut = {(qx, qy)} if what != "v" else {(qx + i, qy + j) for i in (-1, 0, 1) for j in (-1, 0, 1) if 0 <= qx + i < W and 0 <= qy + j < H}
    out, v_out, record = ref.apply(x, v, g, W, H, 1, k, EPS)
    w, N = ref.level_weights(g, record, k, EPS, W, H, 0)
    assert np.isfinite(w).all() and np.isfinite(N).all()
    for t, (i, j) in enumerate(dref.TAPS):
        for y in range(H):
            for xx in range(W):
                ends = ((xx, y) in cut, (xx + i, y + j) in cut)
                inside = 0 <= xx + i < W and 0 <= y + j < H
                if (i, j) != (0, 0) and inside and any(ends):
                    assert w[t][y, xx] == 0.0 and clean[t][y, xx] > 0.0
                else:
                    assert w[t][y, xx] == clean[t][y, xx]
    for (cx, cy) in cut:
        assert w[12][cy, cx] == 36.0 / 256.0 and N[cy, cx] == 36.0 / 256.0
    others = np.arange(W * H) != q
    assert np.isfinite(out[others]).all() and np.isfinite(v_out[others]).all()       # nothing leaks out of q
    xq = x[q].astype(np.float64)
    if what == "x":                                                                   # the centre tap hands q through, the bad value included
        assert np.array_equal(np.isfinite(out[q]), np.isfinite(xq)) and np.all(np.abs(out[q][[0, 2]] - xq[[0, 2]]) <= 4 * 2.0 ** -53 * np.abs(xq[[0, 2]]))
    else:
        assert np.all(np.abs(out[q] - xq) <= 4 * 2.0 ** -53 * np.abs(xq))
    # several levels: the output stays finite away from q
    out5, v5, _ = ref.apply(x, v, g, W, H, 3, k, EPS)
    assert np.isfinite(out5[others]).all() and np.isfinite(v5[others]).all()


def test_restatement_zero_variance():
    """v = 0 everywhere: equal pixels keep weight h h exp(-0) = h h, differing ones get h h exp(-k d^2 / eps)"""
    W, H, k, eps = 7, 5, 0.25, 1e-6
    x = np.zeros((H, W, 1), dtype=np.float32)
    x[:, 4:] = np.float32(1.0e-3)                                               # d = 1e-3: k d^2 / eps = 0.25
    x[:, 6:] = np.float32(1.0)                                                  # d ~ 1: exp(-2.5e5) = 0
    v = np.zeros(W * H, dtype=np.float32)
    _, v_out, record = ref.apply(x.reshape(-1, 1), v, None, W, H, 1, k, eps)
    w, _ = ref.level_weights(None, record, k, eps, W, H, 0)
    d = float(np.float32(1.0e-3))
    for t, (i, j) in enumerate(dref.TAPS):
        hh = dref.H5[i + 2] * dref.H5[j + 2]
        for y in range(H):
            for xx in range(W):
                if not (0 <= xx + i < W and 0 <= y + j < H):
                    continue
                a, b = float(x[y, xx, 0]), float(x[y + j, xx + i, 0])
                if a == b:
                    assert w[t][y, xx] == hh
                elif abs(a - b) < 0.5:
                    assert abs(w[t][y, xx] - hh * np.exp(-k * d * d / eps)) <= 1e-15
                else:
                    assert w[t][y, xx] == 0.0
    assert np.array_equal(v_out, np.zeros(W * H))


# ---------------------------------------------------------------------------------------------------------------------------
# the step frames of the issue, on the restatement
SW, SH = 64, 48
PROTOTYPE_EXACT = (0.0133, 0.0110, 0.0097, 0.0123)          # MSE(out) / MSE(noisy) of the float64 prototype, seeds 0..3
PROTOTYPE_ESTIMATED = (0.053, 0.063, 0.052, 0.062)


def step_clean():
    yy, xx = np.meshgrid(np.arange(SH), np.arange(SW), indexing="ij")
    return np.where(xx + 0.4 * yy < 40, 0.2, 1.0)[..., None] * np.array([1.0, 0.8, 0.6])


def step_exact(seed):
    """(noisy float32 [n, 3], v float32 [n], clean float64 [n, 3]): 10 % relative Gaussian noise and its exact luminance variance"""
    clean = step_clean()
    a = np.array(ref.REC709)
    noisy = clean + 0.1 * clean * np.random.default_rng(seed).standard_normal((SH, SW, 3))
    v = ((a * 0.1 * clean) ** 2).sum(axis=-1)
    return noisy.astype(np.float32).reshape(-1, 3), v.astype(np.float32).reshape(-1), clean.reshape(-1, 3)


def step_estimated(seed):
    """two samples per pixel at 30 % noise; the variance is estimated from them by luminance_variance's rule"""
    clean, n = step_clean(), 2
    a = np.array(ref.REC709)
    smp = clean * (1 + 0.3 * np.sqrt(n) * np.random.default_rng(100 + seed).standard_normal((n, SH, SW, 1)))
    mean, var = smp.mean(axis=0), smp.var(axis=0, ddof=1) / n
    v = (a * np.sqrt(np.maximum(var, 0.0))).sum(axis=-1) ** 2
    return mean.astype(np.float32).reshape(-1, 3), v.astype(np.float32).reshape(-1), clean.reshape(-1, 3)


def mse(a, b):
    return float(((np.asarray(a, np.float64) - b) ** 2).mean())


@pytest.mark.parametrize("seed", range(4))
def test_step_frames_on_the_restatement(seed):
    """the issue's figures, re-measured: had they differed, the operator would have been misread.  The caps are the GPU test's."""
    noisy, v, clean = step_exact(seed)
    out = ref.apply(noisy, v, None, SW, SH, 5, 0.25, EPS)[0]
    plain = dref.apply(noisy, None, SW, SH, 5)
    r, r_plain = mse(out, clean) / mse(noisy, clean), mse(plain, clean) / mse(noisy, clean)
    mean, ve, _ = step_estimated(seed)
    r_est = mse(ref.apply(mean, ve, None, SW, SH, 5, 0.25, EPS)[0], clean) / mse(mean, clean)
    print("seed %d: exact variance %.4f, Denoiser %.2f x the noisy error, estimated variance %.4f" % (seed, r, r_plain, r_est))
    assert abs(r - PROTOTYPE_EXACT[seed]) <= 1e-4 and abs(r_est - PROTOTYPE_ESTIMATED[seed]) <= 1e-3
    assert r <= 1.0 / 40.0 and r_plain > 5.0 and r_est <= 1.0 / 8.0


# ---------------------------------------------------------------------------------------------------------------------------
def test_python_surface_refuses_wrong_arguments(psdr, monkeypatch):
    import torch
    V = psdr.VarianceDenoiser
    with pytest.raises(ValueError, match="guide channels"):
        V(torch.zeros((12, 9)), 4, 3)
    with pytest.raises(ValueError, match="shape"):
        V(torch.zeros((11, 3)), 4, 3)
    with pytest.raises(ValueError, match="levels"):
        V(None, 4, 3, levels=0)
    with pytest.raises(ValueError, match="levels"):
        V(None, 4, 3, levels=9)
    with pytest.raises(ValueError, match="frame"):
        V(None, 0, 3)
    with pytest.raises(ValueError, match="frame"):
        V(None, 4097, 4096)
    for s in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="sigma_l"):
            V(None, 4, 3, sigma_l=s)
    for e in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="eps"):
            V(None, 4, 3, eps=e)
    for a in ((1.0, 2.0), (1.0, float("nan"), 0.0), ()):
        with pytest.raises(ValueError, match="luminance"):
            V(None, 4, 3, luminance=a)
    mean, sq = torch.full((6, 3), 2.0), torch.full((6, 3), 3.0)
    with pytest.raises(ValueError, match="luminance"):
        psdr.luminance_variance(mean, sq, 4, luminance=(1.0,))
    with pytest.raises(ValueError, match="C in"):
        psdr.luminance_variance(torch.zeros((6, 2)), torch.zeros((6, 2)), 4)
    with pytest.raises(ValueError):
        psdr.luminance_variance(mean, sq, 1)
    # (sum_c a_c sqrt(max(var_c, 0)))^2 on the CPU, in float64: var = (3 - 4 / 4) 4 / 3 = 8 / 3 per channel, the coefficients add up to 1
    got = psdr.luminance_variance(mean.double(), sq.double(), 4)
    assert tuple(got.shape) == (6,) and float((got - 8.0 / 3.0).abs().max()) <= 1e-12
    neg = psdr.luminance_variance(torch.tensor([[2.0]]), torch.tensor([[0.5]]), 4)             # sq < mean^2 / n: clamped, not NaN
    assert float(neg) == 0.0
    one = psdr.luminance_variance(torch.tensor([[2.0, 4.0, 0.0]], dtype=torch.float64), torch.tensor([[3.0, 7.0, 0.0]], dtype=torch.float64), 4, luminance=(0.5, 0.25, 9.0))
    assert abs(float(one) - (0.5 * (8.0 / 3.0) ** 0.5 + 0.25 * 4.0 ** 0.5) ** 2) <= 1e-12
    # one GPU only: a clear error before anything is launched
    monkeypatch.setattr(psdr, "_shard", lambda: (0, 2))
    with pytest.raises(RuntimeError, match="one GPU"):
        V(None, 4, 3)
