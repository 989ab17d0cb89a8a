"""The variance-guided a-trous denoiser of include/psdr_hip.h restated in NumPy float64 (tests/test_vdenoise_cpu.py, tests/test_gpu_vdenoise.py).

The float32 inputs are taken as given and every operation runs in float64, as loops over the 25 taps of shifted views of the frame (tests/denoise_ref.py has the taps
and the views).  State (x_l, v_l), x_0 = x, v_0 = v; level l has stride s = 2^l, taps (i, j) in {-2 .. 2}^2, h = [1, 4, 6, 4, 1] / 16:

    lum_l(p) = a_0 x_l,0(p) + a_1 x_l,1(p) + a_2 x_l,2(p)
    vt_l(p)  = 3 x 3 prefilter of v_l at unit stride: [1, 2, 1] x [1, 2, 1] / 16 over the taps inside the frame, divided by the sum of the coefficients that were inside
    q = p + s (i, j) exists only inside the frame;  d2 = sum_k (g_k(p) - g_k(q))^2;  z = k (lum_l(p) - lum_l(q))^2 / (vt_l(p) + vt_l(q) + eps)
    w_l(p, q) = h(i) h(j) exp(-(d2 + z)) if 0 <= d2 + z < inf and vt_l(p) + vt_l(q) + eps is finite, else 0;  the centre tap is h(0)^2;  a tap of weight 0 adds nothing, whatever x(q) and v(q) hold
    N_l(p) = sum_q w_l(p, q);   x_{l+1}(p) = sum_q w_l(p, q) x_l(q) / N_l(p);   v_{l+1}(p) = sum_q w_l(p, q)^2 v_l(q) / N_l(p)^2

The record of an apply is, per level, the planes (lum_l, vt_l, 1 / N_l).  The frozen operator forms the weights from a record - this module's own or one handed in, the
device's for instance - and is linear:  A_l u (p) = (sum_q w_l(p, q) u(q)) (1 / N_l)(p),  A_l^T y (q) = sum_p w_l(q, p) (y(p) (1 / N_l)(p)),  D_x = A_{L-1} ... A_0.
"""
import numpy as np

import denoise_ref as dref

REC709 = (0.2126, 0.7152, 0.0722)
P3 = np.array([1.0, 2.0, 1.0])


def coefficients(a, C):
    if a is None:
        a = REC709 if C == 3 else (1.0,)
    a = np.asarray(a, dtype=np.float32).astype(np.float64)          # the kernel receives them as float32
    assert a.shape == (C,)
    return a


def luminance(f, a):
    """[H, W] from the frame [H, W, C], the terms added in channel order"""
    with np.errstate(invalid="ignore", over="ignore"):
        lum = a[0] * f[..., 0]
        for c in range(1, f.shape[-1]):
            lum = lum + a[c] * f[..., c]
    return lum


def prefilter(v):
    """vt [H, W] from v [H, W]"""
    H, W = v.shape
    acc, norm = np.zeros((H, W)), np.zeros((H, W))
    with np.errstate(invalid="ignore", over="ignore"):
        for j in (-1, 0, 1):
            for i in (-1, 0, 1):
                vw = dref._views(W, H, 1, i, j)
                if vw is None:
                    continue
                p, q = vw
                acc[p] += P3[i + 1] * P3[j + 1] * v[q]
                norm[p] += P3[i + 1] * P3[j + 1]
        return acc / norm


def weights(g, lum, vt, k, eps, W, H, l):
    """(w [25, H, W] in the order of denoise_ref.TAPS, 0 where the tap does not exist; N [H, W]) from the planes lum, vt [H, W]"""
    s = 1 << l
    gg = dref._guides(g, W, H)
    w = np.zeros((25, H, W))
    for t, (i, j) in enumerate(dref.TAPS):
        vw = dref._views(W, H, s, i, j)
        if vw is None:
            continue
        p, q = vw
        if i == 0 and j == 0:
            w[t][p] = dref.H5[2] * dref.H5[2]
            continue
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            d = gg[p] - gg[q]
            d2 = (d * d).sum(axis=-1)
            dl = lum[p] - lum[q]
            den = (vt[p] + vt[q]) + eps
            z = k * (dl * dl) / den
            t_ = d2 + z
            ok = np.isfinite(t_) & (t_ >= 0.0) & np.isfinite(den)
            e = np.where(ok, np.exp(-np.where(ok, t_, 0.0)), 0.0)
        w[t][p] = dref.H5[i + 2] * dref.H5[j + 2] * e
    return w, w.sum(axis=0)


def _gather(src, w, W, H, l, square=False):
    """sum_q w(p, q) src(q) (square: w^2), a tap of weight 0 adding nothing; src [H, W, C]"""
    s = 1 << l
    out = np.zeros_like(src)
    for t, (i, j) in enumerate(dref.TAPS):
        vw = dref._views(W, H, s, i, j)
        if vw is None:
            continue
        p, q = vw
        wt = w[t][p][..., None]
        with np.errstate(invalid="ignore", over="ignore"):
            out[p] += np.where(wt > 0.0, (wt * wt if square else wt) * np.where(wt > 0.0, src[q], 0.0), 0.0)
    return out


def _var_frame(v, W, H):
    v = np.asarray(v)
    assert v.size == W * H
    with np.errstate(invalid="ignore"):
        return v.astype(np.float64).reshape(H, W)


def apply(x, v, g, W, H, L, k, eps, a=None):
    """(x_L [W H, C], v_L [W H], record: a list of L tuples (lum_l, vt_l, 1 / N_l) of [H, W] planes), all float64"""
    f = dref._frame(x, W, H)
    vv = _var_frame(v, W, H)
    a = coefficients(a, f.shape[-1])
    record = []
    for l in range(L):
        lum, vt = luminance(f, a), prefilter(vv)
        w, N = weights(g, lum, vt, k, eps, W, H, l)
        record.append((lum, vt, 1.0 / N))
        with np.errstate(invalid="ignore", over="ignore"):
            f = _gather(f, w, W, H, l) / N[..., None]
            vv = _gather(vv[..., None], w, W, H, l, square=True)[..., 0] / (N * N)
    return f.reshape(W * H, -1), vv.reshape(W * H), record


def record_planes(rec, W, H):
    """a device record [L, 3, W H] (float32) as this module's list of float64 [H, W] planes"""
    rec = np.asarray(rec)
    return [tuple(rec[l, i].astype(np.float64).reshape(H, W) for i in range(3)) for l in range(rec.shape[0])]


def level_weights(g, record, k, eps, W, H, l):
    lum, vt, _ = record[l]
    return weights(g, lum, vt, k, eps, W, H, l)


def frozen(u, g, record, W, H, k, eps):
    """D_x u: [W H, C] float64"""
    f = dref._frame(u, W, H)
    for l in range(len(record)):
        w, _ = level_weights(g, record, k, eps, W, H, l)
        f = _gather(f, w, W, H, l) * record[l][2][..., None]
    return f.reshape(W * H, -1)


def frozen_adj(y, g, record, W, H, k, eps):
    """D_x^T y: [W H, C] float64"""
    f = dref._frame(y, W, H)
    for l in range(len(record) - 1, -1, -1):
        w, _ = level_weights(g, record, k, eps, W, H, l)
        f = _gather(f * record[l][2][..., None], w, W, H, l)          # (the transpose gathers with w(q', p') of the SAME pair: w is symmetric)
    return f.reshape(W * H, -1)
