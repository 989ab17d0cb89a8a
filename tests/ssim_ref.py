"""The float64 checker of the SSIM loss (include/psdr_hip.h, section "THE SSIM LOSS"): taps, window sum, loss, mean, map and gradient, and the rigorous float32 error
bound tests/test_gpu_ssim.py holds the kernels to.  numpy only.

    img = x, target = y [W H, C], pixel (x, y) at row y W + x; mask None, [W H] or [W H, 1]
    G v = vertical pass of (horizontal pass of v), each sum_k g_k v(. + k - R), zeros outside the frame
    mu_x = G x, mu_y = G y, s_xx = G(x x) - mu_x mu_x, s_yy likewise, s_xy = G(x y) - mu_x mu_y
    a1 = 2 (mu_x mu_y) + C1, a2 = 2 s_xy + C2, b1 = (mu_x mu_x + mu_y mu_y) + C1, b2 = (s_xx + s_yy) + C2, S = (a1 a2) / (b1 b2)
    N = C sum m_eff, mean = sum m_eff S / N, loss = 1 - mean  (N == 0: loss = mean = 0, gradient 0)
    P = m_eff [2 mu_y (a2 - a1) - 2 mu_x S (b2 - b1)] / (b1 b2), Q = -m_eff S / b2, T = m_eff 2 a1 / (b1 b2)
    dloss / dimg = -(G P + 2 x G Q + y G T) / N

THE BOUND (bounds()).  u = 2^-24, gamma_m = m u / (1 - m u).  Every float32 operation returns its exact result times (1 + d), |d| <= u, and a product, quotient or
fma whose result falls below 2^-126 is off by at most eta = 2^-149 more (gradual underflow: the kernels are built without flushing denormals; sums and differences
underflow exactly).  eta matters where a window of sigma = 0.5 multiplies by taps of 1e-22 twice.  An explicit fma has fewer roundings than the product and sum it
replaces, so it stays inside.
  window sum   two passes of K products and K - 1 additions each: every term is rounded at most 2 K times whatever the order, so |fl(G v) - G v| <= gamma_{2K} G|v| + 2 K eta;
               on inputs that carry a bound e themselves: G e + gamma_{2K} G(|v| + e) + 2 K eta.  x x and x y are one rounding before the sum.
  propagation  a value-with-bound arithmetic (class VB): an operation on (a, ea), (b, eb) gives the exact result of a and b with the bound e0 of the exact result of
               the computed operands (ea + eb for a sum, |a| eb + |b| ea + ea eb for a product, (ea + |q| eb) / (|b| - eb) for a quotient q, |b| - eb asserted
               positive) plus the rounding u (|result| + e0), and eta for a product or quotient.  Factors 2 and signs are exact.  Rigorous, not first-order.
  sums         n terms added in any order: sum of their bounds + gamma_{n-1} sum (|t| + e_t).
The formula is pushed through in the order the header states it; the kernels evaluate it in that order (csrc/hip/ssim.hip).  The float64 values the bounds are taken
around carry float64's own rounding, 2^-29 of u: not counted.

Images are handled as [H, W, C] arrays inside; every function takes and returns the flat [W H, C] layout."""
import math

import numpy as np

U = 2.0 ** -24
ETA = 2.0 ** -149          # the smallest subnormal float32: what an underflowing product, quotient or fma can lose


def gamma(m):
    m = np.asarray(m, np.float64)
    return m * U / (1.0 - m * U)


def taps(size=11, sigma=1.5):
    """the float32 taps, the definition: exp(-(k - R)^2 / (2 sigma^2)) normalised in double, rounded once"""
    r = size // 2
    g = [math.exp(-float((k - r) * (k - r)) / (2.0 * sigma * sigma)) for k in range(size)]
    total = sum(g)
    return np.array([v / total for v in g], dtype=np.float64).astype(np.float32)


def constants(data_range=1.0, k1=0.01, k2=0.03):
    """(C1, C2), each rounded once to float32"""
    return np.float32((k1 * data_range) ** 2), np.float32((k2 * data_range) ** 2)


def window_sum(v, g, shift=0):
    """G v for v [H, W, C] in v's dtype: horizontal pass, then vertical pass, zeros outside.  shift: the window displaced by that many pixels in both directions (a
    deliberately wrong halo, for the detection-power test)"""
    v = np.asarray(v)
    g = np.asarray(g).astype(v.dtype)
    K = len(g)
    R = K // 2
    H, W, C = v.shape
    pad = R + abs(shift)
    p = np.zeros((H, W + 2 * pad, C), v.dtype)
    p[:, pad:pad + W] = v
    h = np.zeros_like(v)
    for k in range(K):
        o = pad + k - R + shift
        h = h + g[k] * p[:, o:o + W]
    p = np.zeros((H + 2 * pad, W, C), v.dtype)
    p[pad:pad + H] = h
    out = np.zeros_like(v)
    for k in range(K):
        o = pad + k - R + shift
        out = out + g[k] * p[o:o + H]
    return out


def effective_mask(width, height, window, mask=None, padding="same"):
    """m_eff [H, W, 1] in float64"""
    m = np.ones((height, width, 1)) if mask is None else np.asarray(mask, np.float64).reshape(height, width, 1)
    if padding == "valid":
        R = window // 2
        inside = np.zeros((height, width, 1))
        inside[R:height - R, R:width - R] = 1.0
        m = m * inside
    else:
        assert padding == "same"
    return m


def evaluate(img, target, width, height, window=11, sigma=1.5, data_range=1.0, k1=0.01, k2=0.03, mask=None, padding="same", g=None, shift=0, dtype=np.float64):
    """(loss, mean, S [W H, C], dloss / dimg [W H, C]) in `dtype` (float32: the arithmetic of the kernels in one particular summation order).  g: other taps than
    taps(window, sigma); shift: see window_sum"""
    g = taps(window, sigma) if g is None else g
    x = np.asarray(img, dtype).reshape(height, width, -1)
    y = np.asarray(target, dtype).reshape(height, width, -1)
    C = x.shape[2]
    c1, c2 = (dtype(c) for c in constants(data_range, k1, k2))
    G = lambda v: window_sum(v, g, shift)
    two = dtype(2)
    mx, my = G(x), G(y)
    mxx, myy, mxy = mx * mx, my * my, mx * my
    sxx, syy, sxy = G(x * x) - mxx, G(y * y) - myy, G(x * y) - mxy
    a1, a2 = two * mxy + c1, two * sxy + c2
    b1, b2 = (mxx + myy) + c1, (sxx + syy) + c2
    den = b1 * b2
    S = (a1 * a2) / den
    m = effective_mask(width, height, window, mask, padding).astype(dtype)
    N = dtype(C) * m.sum(dtype=dtype)
    if not N > 0:
        return dtype(0), dtype(0), S.reshape(-1, C), np.zeros((width * height, C), dtype)
    mean = (m * S).sum(dtype=dtype) / N
    P = m * (((two * my) * (a2 - a1) - ((two * mx) * S) * (b2 - b1)) / den)
    Q = -(m * (S / b2))
    T = m * ((two * a1) / den)
    grad = ((G(P) + (two * x) * G(Q)) + y * G(T)) * -(dtype(1) / N)
    return dtype(1) - mean, mean, S.reshape(-1, C), grad.reshape(-1, C)


class VB:
    """a float64 value (array) and a bound on |what float32 computed - value|"""

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, np.float64)
        self.e = np.broadcast_to(np.asarray(e, np.float64), self.v.shape)

    def _round(self, v, e0, eta=0.0):
        return VB(v, e0 + U * (np.abs(v) + e0) + eta)

    def __add__(self, o):
        return self._round(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        return self._round(self.v - o.v, self.e + o.e)

    def __mul__(self, o):
        return self._round(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e, ETA)

    def __truediv__(self, o):
        low = np.abs(o.v) - o.e
        assert np.all(low > 0), "a denominator's lower bound is not positive"
        q = self.v / o.v
        return self._round(q, (self.e + np.abs(q) * o.e) / low, ETA)

    def __neg__(self):
        return VB(-self.v, self.e)

    def twice(self):
        return VB(2.0 * self.v, 2.0 * self.e)


def _vb_window_sum(a, g):
    g64 = np.asarray(g, np.float64)
    return VB(window_sum(a.v, g64), window_sum(a.e, g64) + gamma(2 * len(g)) * window_sum(np.abs(a.v) + a.e, g64) + 2 * len(g) * ETA)


def _vb_sum(t):
    n = t.v.size
    return VB(t.v.sum(), t.e.sum() + gamma(max(n - 1, 0)) * (np.abs(t.v) + t.e).sum())


def bounds(img, target, width, height, window=11, sigma=1.5, data_range=1.0, k1=0.01, k2=0.03, mask=None, padding="same"):
    """{name: VB} for S, P, Q, T, grad ([W H, C] each), mean and loss (0-d): the float64 values and the bounds float32 kernels must stay within.  img, target and mask
    must hold float32 values (they are exact inputs)."""
    g = taps(window, sigma)
    x = VB(np.asarray(img, np.float64).reshape(height, width, -1))
    y = VB(np.asarray(target, np.float64).reshape(height, width, -1))
    C = x.v.shape[2]
    c1, c2 = (VB(np.float64(c)) for c in constants(data_range, k1, k2))
    G = lambda a: _vb_window_sum(a, g)
    mx, my = G(x), G(y)
    mxx, myy, mxy = mx * mx, my * my, mx * my
    sxx, syy, sxy = G(x * x) - mxx, G(y * y) - myy, G(x * y) - mxy
    a1, a2 = mxy.twice() + c1, sxy.twice() + c2
    b1, b2 = (mxx + myy) + c1, (sxx + syy) + c2
    den = b1 * b2
    S = (a1 * a2) / den
    m = VB(effective_mask(width, height, window, mask, padding))
    flat = lambda a: VB(a.v.reshape(-1, C), a.e.reshape(-1, C))
    P = m * ((my.twice() * (a2 - a1) - (mx.twice() * S) * (b2 - b1)) / den)
    Q = -(m * (S / b2))
    T = m * (a1.twice() / den)
    res = {"S": flat(S), "P": flat(P), "Q": flat(Q), "T": flat(T)}
    msum = _vb_sum(m)
    N = VB(float(C)) * msum
    if not N.v > 0:
        zero = VB(np.zeros((width * height, C)))
        res.update(mean=VB(0.0), loss=VB(0.0), grad=zero)
        return res
    mean = _vb_sum(m * S) / N
    scale = -(VB(1.0) / N)
    grad = ((G(P) + x.twice() * G(Q)) + y * G(T)) * scale
    res.update(mean=mean, loss=VB(1.0) - mean, grad=flat(grad))
    return res


def uniform_inputs(width, height, channels, seed=0):
    """(img, target) float32 [W H, C], uniform in [0, 1)"""
    rng = np.random.default_rng([seed, width, height, channels])
    n = width * height
    return rng.random((n, channels), dtype=np.float32), rng.random((n, channels), dtype=np.float32)


def flat_inputs(width, height, channels, seed=0):
    """(img, target) float32: 0.6 + 0.02 sin + 0.002 noise, nearly flat - E_xx - mu_x^2 cancels against C2"""
    rng = np.random.default_rng([seed + 100, width, height, channels])
    yy, xx = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    out = []
    for phase in (0.0, 0.7):
        base = 0.6 + 0.02 * np.sin(0.31 * xx + 0.17 * yy + phase)[:, :, None] + 0.002 * rng.standard_normal((height, width, channels))
        out.append(base.reshape(-1, channels).astype(np.float32))
    return out[0], out[1]


def masks(width, height, seed=0):
    """(a mask with about a quarter zeros, a fractional mask) float32 [W H, 1].  The zeros come in blocks, so that on frames larger than the window some masked pixels
    have no unmasked pixel within R"""
    rng = np.random.default_rng([seed + 200, width, height])
    n = width * height
    zeros = (rng.random((height, width)) < 0.08)
    yy, xx = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    block = (xx >= width // 4) & (xx < width // 4 + max(1, (2 * width) // 5)) & (yy >= height // 4) & (yy < height // 4 + max(1, (2 * height) // 5))
    binary = 1.0 - (zeros | block).astype(np.float32)
    frac = (rng.integers(0, 5, (height, width)) / 4.0).astype(np.float32)
    return binary.reshape(n, 1), frac.reshape(n, 1)
