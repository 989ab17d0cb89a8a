"""The float64 checker of the multi-scale image loss (include/psdr_hip.h, section "MULTI-SCALE IMAGE LOSS"): pyramid, losses, gradient and the terms the error
bounds of tests/test_gpu_msloss.py are taken over.  numpy only.

    img, target [W H, C], pixel (x, y) at row y W + x; weight None, [W H], [W H, 1] or [W H, C]
    d_0 = weight (img - target);  d_{l+1}(i, j) = the mean of those of d_l(2i .. 2i + 1, 2j .. 2j + 1) that exist
    level_loss_l = sum rho(d_l) / (C W_l H_l);  loss = sum_l lambda_l level_loss_l;  rho = |x| (rho'(0) = 0) or x^2
    dloss / dimg = weight G_0,  G_l = (lambda_l / (C W_l H_l)) rho'(d_l) + P_{l+1}^T G_{l+1}

Images are handled as [H, W, C] arrays inside; every function takes and returns the flat [W H, C] layout."""
import numpy as np


def shapes(width, height, levels=None):
    out = [(int(width), int(height))]
    while out[-1] != (1, 1):
        out.append(((out[-1][0] + 1) // 2, (out[-1][1] + 1) // 2))
    return out if levels is None else out[:levels]


def _counts(h, w):
    """[ceil(h / 2), ceil(w / 2)]: how many pixels of an h x w level lie under each pixel of the next"""
    cy = np.minimum(2, h - 2 * np.arange((h + 1) // 2))
    cx = np.minimum(2, w - 2 * np.arange((w + 1) // 2))
    return cy[:, None] * cx[None, :]


def pool(x, dtype=np.float64):
    """one level up: x [h, w, C] -> [ceil(h / 2), ceil(w / 2), C], ((a + b) + (c + d)) / count with missing pixels as 0, in `dtype`"""
    h, w, C = x.shape
    p = np.zeros((2 * ((h + 1) // 2), 2 * ((w + 1) // 2), C), dtype)
    p[:h, :w] = x
    s = (p[0::2, 0::2] + p[0::2, 1::2]) + (p[1::2, 0::2] + p[1::2, 1::2])
    return (s * (1.0 / _counts(h, w))[:, :, None].astype(dtype)).astype(dtype)


def unpool(g, h, w):
    """the transpose of pool: g [ceil(h / 2), ceil(w / 2), C] -> [h, w, C], every child gets its parent's value / count"""
    q = g / _counts(h, w)[:, :, None]
    return np.repeat(np.repeat(q, 2, axis=0), 2, axis=1)[:h, :w]


def _weight(weight, n, C):
    if weight is None:
        return np.ones((n, 1))
    w = np.asarray(weight, np.float64)
    return w.reshape(n, -1)


def pyramid(img, target, width, height, weight=None, levels=None, dtype=np.float64):
    """[d_l as [W_l H_l, C]] in `dtype` (float32: the arithmetic of the kernels, for the exactness check of the test inputs)"""
    img, target = np.asarray(img, dtype), np.asarray(target, dtype)
    n, C = img.shape
    d = (_weight(weight, n, C).astype(dtype) * (img - target)).astype(dtype).reshape(height, width, C)
    out = [d]
    for _ in range(len(shapes(width, height, levels)) - 1):
        out.append(pool(out[-1], dtype))
    return [x.reshape(-1, C) for x in out]


def rho(d, norm):
    return np.abs(d) if norm == "l1" else d * d


def drho(d, norm):
    return np.sign(d) if norm == "l1" else 2.0 * d


def losses(pyr, norm, level_weights=None):
    """(loss, [level_loss_l]) of a pyramid (float64 arithmetic on whatever values it holds)"""
    lam = np.ones(len(pyr)) if level_weights is None else np.asarray(level_weights, np.float64)
    ll = np.array([rho(np.asarray(d, np.float64), norm).sum() / d.size for d in pyr])
    return float((lam * ll).sum()), ll


def gradient_terms(pyr, width, height, norm, weight=None, level_weights=None):
    """[term_l as [W H, C]]: level l's contribution to dloss / dimg, weight P_1^T .. P_l^T (lambda_l / (C W_l H_l)) rho'(d_l); their sum is the gradient"""
    shp = shapes(width, height, len(pyr))
    C = pyr[0].shape[1]
    lam = np.ones(len(pyr)) if level_weights is None else np.asarray(level_weights, np.float64)
    w = _weight(weight, width * height, C)
    terms = []
    for l, d in enumerate(pyr):
        wl, hl = shp[l]
        g = (lam[l] / d.size) * drho(np.asarray(d, np.float64), norm).reshape(hl, wl, C)
        for k in range(l, 0, -1):
            g = unpool(g, shp[k - 1][1], shp[k - 1][0])
        terms.append(w * g.reshape(-1, C))
    return terms


def evaluate(img, target, width, height, norm, weight=None, levels=None, level_weights=None):
    """(loss, level losses, dloss / dimg [W H, C], pyramid) in float64"""
    pyr = pyramid(img, target, width, height, weight, levels)
    loss, ll = losses(pyr, norm, level_weights)
    return loss, ll, sum(gradient_terms(pyr, width, height, norm, weight, level_weights)), pyr


def footprint_mean_abs(img, target, width, height, weight=None, levels=None):
    """[the level-l mean of |d_0| over each pixel's footprint]: the pyramid of |d_0|"""
    n, C = np.asarray(img).shape
    a = np.abs(_weight(weight, n, C) * (np.asarray(img, np.float64) - np.asarray(target, np.float64)))
    return pyramid(a, np.zeros_like(a), width, height, None, levels)
