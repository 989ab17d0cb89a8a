"""The a-trous denoiser, what can be checked without a GPU: the entry points are declared, exported and listed and the ABI did not move; every entry point refuses bad
arguments before it touches a device; the float64 restatement (tests/denoise_ref.py, which tests/test_gpu_denoise.py compares the kernels against) has the properties
the specification promises; the Python surface refuses wrong shapes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import denoise_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("psdr_hip_denoise_create", "psdr_hip_denoise_apply", "psdr_hip_denoise_apply_adj", "psdr_hip_denoise_destroy")


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
        assert re.search(r"^int\s+%s\s*\(" % name, text, re.M), "%s is not declared in include/psdr_hip.h" % name
        assert hasattr(L, name), "libpsdr_hip.so does not export %s" % name
        assert name in cabi.SYMBOLS
        assert getattr(L, name).argtypes is not None, "%s has no argtypes" % name
    assert re.search(r"#define\s+PSDR_HIP_ABI_VERSION\s+16\b", text)
    assert L.psdr_hip_abi_version() == 16
    for name in ("Denoiser", "first_hit_guides"):
        assert hasattr(psdr, name)


def test_every_entry_point_refuses_bad_arguments_before_any_device_call(psdr):
    """no GPU is visible here: a call that reached the device would fail with a HIP error, not with the entry point's own message.  The non-NULL pointers are host
    addresses that a refused call never reads."""
    from psdr_jit_amd import cabi
    L = cabi.lib()
    host = np.zeros(64, dtype=np.int64)
    p, p2 = host.ctypes.data, host.ctypes.data + 64

    def refused(rc, name, word):
        msg = L.psdr_hip_last_error().decode()
        assert rc != 0 and msg.startswith(name + ":") and word in msg and "hip" not in msg[len(name):].lower(), (name, word, rc, msg)

    name = "psdr_hip_denoise_create"
    h = C.c_void_p()
    refused(L.psdr_hip_denoise_create(p, 3, 16, 16, 5, None, None), name, "NULL")
    refused(L.psdr_hip_denoise_create(None, 3, 16, 16, 5, C.byref(h), None), name, "NULL")
    for W, H, word in ((0, 16, "W = 0"), (16, 0, "H = 0"), (-3, 16, "W = -3"), (16, -1, "H = -1"), (4097, 4096, "2^24"), (1 << 24, 2, "2^24"), (1 << 30, 1 << 30, "2^24")):
        refused(L.psdr_hip_denoise_create(p, 3, W, H, 5, C.byref(h), None), name, word)
    for Lv in (0, -1, 9):
        refused(L.psdr_hip_denoise_create(p, 3, 16, 16, Lv, C.byref(h), None), name, "L = %d" % Lv)
    for G in (-1, 9):
        refused(L.psdr_hip_denoise_create(p, G, 16, 16, 5, C.byref(h), None), name, "G = %d" % G)
    assert not h.value                                        # a refused create leaves no handle behind

    fake = C.c_void_p(p)                                      # (a refused call never looks into the handle)
    for name in ("psdr_hip_denoise_apply", "psdr_hip_denoise_apply_adj"):
        fn = getattr(L, name)
        refused(fn(None, p, 3, p2, None), name, "NULL")
        refused(fn(fake, None, 3, p2, None), name, "NULL")
        refused(fn(fake, p, 3, None, None), name, "NULL")
        refused(fn(fake, p, 0, p2, None), name, "C must")
        refused(fn(fake, p, 5, p2, None), name, "C must")
        refused(fn(fake, p, 3, p, None), name, "different")
    refused(L.psdr_hip_denoise_destroy(None), "psdr_hip_denoise_destroy", "NULL")


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement's own properties, in float64
def _guides(rng, W, H, G):
    """pre-scaled guides, float32 [W H, G], whose differences give d2 from exactly 0 (a patch of equal values) to beyond 100 (a step of 11 in every third channel,
    the first included): smooth ramps, steps, noise of a fraction of a unit and of a few units"""
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    g = np.zeros((H, W, G), dtype=np.float32)
    for k in range(G):
        g[..., k] = 0.05 * xx + 0.02 * yy if k % 2 == 0 else 0.3 * rng.standard_normal((H, W))
        if k % 3 == 0:
            g[..., k] += 11.0 * (xx > W // 2)
        if k % 4 == 2:
            g[..., k] += 3.0 * rng.standard_normal((H, W))
    g[:H // 2, :W // 3, :] = 0.25
    return g.reshape(W * H, G)


def _dense(g, W, H, l):
    """A_l as a dense [n, n] matrix, and w_l"""
    w, N = ref.weights(g, W, H, l)
    n, s = W * H, 1 << l
    Wm = np.zeros((n, n))
    for t, (i, j) in enumerate(ref.TAPS):
        for y in range(H):
            for x in range(W):
                qx, qy = x + s * i, y + s * j
                if 0 <= qx < W and 0 <= qy < H:
                    Wm[y * W + x, qy * W + qx] += w[t][y, x]
                else:
                    assert w[t][y, x] == 0.0          # a tap outside the frame is dropped
    return Wm / N.reshape(n, 1), Wm


@pytest.mark.parametrize("W,H,G", [(1, 1, 0), (5, 3, 2), (9, 7, 0), (9, 7, 8), (13, 6, 3)])
def test_restatement_rows_symmetry_and_matrix_form(W, H, G):
    rng = np.random.default_rng(W * 100 + H * 10 + G)
    g = _guides(rng, W, H, G) if G else None
    x = rng.standard_normal((W * H, 3))
    D = np.eye(W * H)
    for l in range(4):
        A, Wm = _dense(g, W, H, l)
        assert np.abs(A.sum(axis=1) - 1.0).max() <= 1e-14                     # row-stochastic
        assert np.array_equal(Wm, Wm.T)                                      # w_l(p, q) = w_l(q, p), bit for bit
        assert (ref.weights(g, W, H, l)[1] >= 9.0 / 64.0).all()
        D = A @ D
        assert np.abs(ref.apply(x, g, W, H, l + 1) - D @ x).max() <= 1e-13 * np.abs(x).max()
        assert np.abs(ref.apply_adj(x, g, W, H, l + 1) - D.T @ x).max() <= 1e-12 * np.abs(x).max()


@pytest.mark.parametrize("W,H,L,G,C", [(33, 9, 5, 8, 3), (67, 35, 5, 1, 4), (5, 3, 3, 0, 1), (64, 17, 4, 8, 1)])
def test_restatement_transpose_identity(W, H, L, G, C):
    rng = np.random.default_rng(7 + W)
    g = _guides(rng, W, H, G) if G else None
    x, y = rng.standard_normal((W * H, C)), rng.standard_normal((W * H, C))
    lhs, rhs = (ref.apply(x, g, W, H, L) * y).sum(), (x * ref.apply_adj(y, g, W, H, L)).sum()
    assert abs(lhs - rhs) <= 1e-12 * (np.abs(x) * np.abs(y)).sum()


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("where", ["interior", "corner"])
def test_restatement_non_finite_guide(bad, where):
    """a non-finite guide value at q zeroes exactly the taps that touch q and leaves q's own centre tap"""
    W, H, G = 11, 9, 3
    rng = np.random.default_rng(3)
    g = _guides(rng, W, H, G) * 0.1                                            # (small differences: every other weight is well above 0)
    qx, qy = (5, 4) if where == "interior" else (0, 0)
    clean = [ref.weights(g, W, H, l)[0] for l in range(3)]
    g[qy * W + qx, 1] = bad
    for l in range(3):
        w, N = ref.weights(g, W, H, l)
        s = 1 << l
        assert np.isfinite(w).all() and np.isfinite(N).all()
        for t, (i, j) in enumerate(ref.TAPS):
            for y in range(H):
                for x in range(W):
                    touches = ((x, y) == (qx, qy)) != ((x + s * i, y + s * j) == (qx, qy))          # one end of the tap is q, and it is not q's centre tap
                    inside = 0 <= x + s * i < W and 0 <= y + s * j < H
                    if touches and inside:
                        assert w[t][y, x] == 0.0 and clean[l][t][y, x] > 0.0
                    else:
                        assert w[t][y, x] == clean[l][t][y, x]
        assert w[12][qy, qx] == 36.0 / 256.0 and N[qy, qx] == 36.0 / 256.0       # q keeps its centre tap, and nothing else
    x = rng.standard_normal((W * H, 2))
    out = ref.apply(x, g, W, H, 3)
    # q passes through every level: x h(0)^2 / h(0)^2, two roundings per level (9 is not a power of two)
    assert np.isfinite(out).all() and np.all(np.abs(out[qy * W + qx] - x[qy * W + qx]) <= 3 * 2 * 2.0 ** -53 * np.abs(x[qy * W + qx]))


def test_restatement_strides_beyond_the_frame_give_the_identity():
    W, H = 3, 2
    rng = np.random.default_rng(5)
    g = _guides(rng, W, H, 4)
    x = rng.standard_normal((W * H, 3))
    for l in (2, 3, 7):                                                        # stride 4 and up: no tap but the centre lies inside a 3 x 2 frame
        w, N = ref.weights(g, W, H, l)
        assert np.array_equal(N, np.full((H, W), 36.0 / 256.0)) and np.count_nonzero(w) == W * H
    # level by level: A_l x = (h(0)^2 x) / h(0)^2 - one multiplication and one division by the same power-of-two multiple of 9, exact or not they cancel to within
    # two roundings; the identity is exact in exact arithmetic, which is what 1e-15 relative states
    lo = ref.apply(x, g, W, H, 2)
    hi = ref.apply(x, g, W, H, 8)
    assert np.abs(hi - lo).max() <= 12 * 2.0 ** -53 * np.abs(lo).max()
    one = np.ones((1, 2))
    assert np.abs(ref.apply(one * 3.25, None, 1, 1, 8) - 3.25).max() <= 16 * 2.0 ** -53 * 3.25       # a 1 x 1 frame: every level is the identity


def test_python_surface_refuses_wrong_shapes(psdr, monkeypatch):
    import torch
    with pytest.raises(ValueError, match="guide channels"):
        psdr.Denoiser(torch.zeros((12, 9)), 4, 3)
    with pytest.raises(ValueError, match="shape"):
        psdr.Denoiser(torch.zeros((11, 3)), 4, 3)
    with pytest.raises(ValueError, match="shape"):
        psdr.Denoiser(torch.zeros(12), 4, 3)
    with pytest.raises(ValueError, match="levels"):
        psdr.Denoiser(None, 4, 3, levels=0)
    with pytest.raises(ValueError, match="levels"):
        psdr.Denoiser(None, 4, 3, levels=9)
    with pytest.raises(ValueError, match="frame"):
        psdr.Denoiser(None, 0, 3)
    with pytest.raises(ValueError, match="frame"):
        psdr.Denoiser(None, 4097, 4096)
    with pytest.raises(ValueError, match="channels"):
        psdr.first_hit_guides(None, fields=("silhouette", "shNormal", "position", "bsdf"))           # 1 + 3 + 3 + 3 = 10
    with pytest.raises(ValueError, match="channels"):
        psdr.first_hit_guides(None, fields=("position", "geoNormal", "shNormal"))
    with pytest.raises(ValueError, match="unknown field"):
        psdr.first_hit_guides(None, fields=("albedo",))
    with pytest.raises(ValueError, match="sigma"):
        psdr.first_hit_guides(None, fields=("depth",), sigma={"depth": 0.0})
    with pytest.raises(ValueError, match="sigma"):
        psdr.first_hit_guides(None, fields=("depth",), sigma={"uv": 1.0})
    with pytest.raises(ValueError, match="no field"):
        psdr.first_hit_guides(None, fields=())
    # one GPU only: a clear error before anything is launched
    monkeypatch.setattr(psdr, "_shard", lambda: (0, 2))
    with pytest.raises(RuntimeError, match="one GPU"):
        psdr.Denoiser(None, 4, 3)
    with pytest.raises(RuntimeError, match="one GPU"):
        psdr.first_hit_guides(None)
