"""The edge-avoiding a-trous denoiser of include/psdr_hip.h restated in NumPy float64 (tests/test_denoise_cpu.py, tests/test_gpu_denoise.py).

The float32 guides are taken as given and every operation runs in float64, as loops over the 25 taps of shifted views of the frame:

    level l has stride s = 2^l, taps (i, j) in {-2 .. 2}^2, h = [1, 4, 6, 4, 1] / 16
    q = p + s (i, j) exists only inside the frame;  d2 = sum_k (g_k(p) - g_k(q))^2;  w_l(p, q) = h(i) h(j) exp(-d2) if d2 is finite, else 0;  the centre tap is h(0)^2
    N_l(p) = sum_q w_l(p, q);   A_l x (p) = sum_q w_l(p, q) x(q) / N_l(p);   D = A_{L-1} ... A_0
    A_l^T y (q) = sum_p w_l(q, p) (y(p) / N_l(p)) - w_l is symmetric;   D^T = A_0^T ... A_{L-1}^T
"""
import numpy as np

H5 = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
TAPS = [(i, j) for j in range(-2, 3) for i in range(-2, 3)]          # the order the kernel adds them in: row by row


def _views(W, H, s, i, j):
    """(slices of p, slices of q = p + s (i, j)) over the [H, W] frame for the pixels p whose tap exists, or None when no pixel has it"""
    dx, dy = s * i, s * j
    if abs(dx) >= W or abs(dy) >= H:
        return None
    px = slice(max(0, -dx), W - max(0, dx))
    py = slice(max(0, -dy), H - max(0, dy))
    qx = slice(max(0, dx), W - max(0, -dx))
    qy = slice(max(0, dy), H - max(0, -dy))
    return (py, px), (qy, qx)


def _guides(g, W, H):
    if g is None:
        return np.zeros((H, W, 0))
    g = np.asarray(g)
    assert g.shape[0] == W * H and g.ndim == 2
    with np.errstate(invalid="ignore"):
        return g.astype(np.float64).reshape(H, W, g.shape[1])


def weights(g, W, H, l):
    """(w [25, H, W] in the order of TAPS - w[t][y, x] is the weight of tap t of pixel (x, y), 0 where the tap does not exist; N [H, W])"""
    s = 1 << l
    gg = _guides(g, W, H)
    w = np.zeros((25, H, W))
    for t, (i, j) in enumerate(TAPS):
        v = _views(W, H, s, i, j)
        if v is None:
            continue
        p, q = v
        if i == 0 and j == 0:
            w[t][p] = H5[2] * H5[2]
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            d = gg[p] - gg[q]
            d2 = (d * d).sum(axis=-1)
            e = np.where(np.isfinite(d2), np.exp(-np.where(np.isfinite(d2), d2, 0.0)), 0.0)
        w[t][p] = H5[i + 2] * H5[j + 2] * e
    return w, w.sum(axis=0)


def _level(x, w, N, W, H, l, adjoint):
    s = 1 << l
    src = x / N[..., None] if adjoint else x
    out = np.zeros_like(x)
    for t, (i, j) in enumerate(TAPS):
        v = _views(W, H, s, i, j)
        if v is None:
            continue
        p, q = v
        out[p] += w[t][p][..., None] * src[q]          # (the transpose gathers with w(q', p') of the SAME pair: w is symmetric)
    return out if adjoint else out / N[..., None]


def _frame(x, W, H):
    x = np.asarray(x)
    assert x.ndim == 2 and x.shape[0] == W * H
    return x.astype(np.float64).reshape(H, W, x.shape[1])


def apply(x, g, W, H, L):
    """D x: [W H, C] float64"""
    f = _frame(x, W, H)
    for l in range(L):
        w, N = weights(g, W, H, l)
        f = _level(f, w, N, W, H, l, False)
    return f.reshape(W * H, -1)


def apply_adj(y, g, W, H, L):
    """D^T y: [W H, C] float64"""
    f = _frame(y, W, H)
    for l in range(L - 1, -1, -1):
        w, N = weights(g, W, H, l)
        f = _level(f, w, N, W, H, l, True)
    return f.reshape(W * H, -1)
