"""The SSIM loss: 1 - the mean structural similarity of two images under a Gaussian window, value and image gradient in one fused pass (DESIGN.md section 7i;
kernels: csrc/hip/ssim.hip).

A norm of pixel differences cannot tell structure from brightness: a slightly blurred texture and a slightly shifted exposure cost the same, and residual Monte-Carlo
or denoiser blur is rewarded.  SSIM compares local means, variances and the covariance; inverse-rendering pipelines add it to a pixel norm:

    ms = psdr.MultiScaleLoss(sc.opts.width, sc.opts.height)
    ss = psdr.SSIMLoss(sc.opts.width, sc.opts.height)                    # channels=3, an 11-tap Gaussian window of sigma 1.5, data_range=1
    loss = (1 - a) * ms(img, target) + a * ss(img, target)

The definition (include/psdr_hip.h states it in full).  img = x, target = y [W H, C], pixel (x, y) at row y W + x; mask m absent, [W H] or [W H, 1], without gradient.
G v is the K x K window sum of v with the taps of gaussian_window(K, sigma), pixels outside the frame counting as 0 (F.conv2d(padding=K // 2)).  mu_x = G x, mu_y = G y,
s_xx = G(x x) - mu_x^2, s_yy likewise, s_xy = G(x y) - mu_x mu_y;  S = ((2 mu_x mu_y + C1) (2 s_xy + C2)) / ((mu_x^2 + mu_y^2 + C1) (s_xx + s_yy + C2)) with
C1 = (k1 data_range)^2, C2 = (k2 data_range)^2;  loss = 1 - sum m_eff S / (C sum m_eff), m_eff = m ("same") or m on the pixels whose window lies wholly inside the
frame and 0 elsewhere ("valid", Wang et al.'s form).  Three launches give the loss, the mean and dloss / dimg; the gradient is a gather (the window is symmetric), no
atomics: the same input gives the same bits.

SSIM assumes a bounded range: tone-map HDR renders into [0, data_range] first.  One GPU only: under an initialised torch.distributed group of more than one rank the
calls raise."""
import ctypes as _C
import functools as _functools
import math as _math

from ._opcommon import _single_gpu

PADDINGS = {"same": 0, "valid": 1}          # PSDR_SSIM_SAME, PSDR_SSIM_VALID
MAX_CHANNELS, MAX_SIDE, MAX_PIXELS = 4, 16384, 1 << 24
MIN_WINDOW, MAX_WINDOW = 3, 11


def gaussian_window(size=11, sigma=1.5):
    """float32 numpy [size]: g_k = exp(-(k - R)^2 / (2 sigma^2)), R = size // 2, normalised in double and rounded once.  These taps are the definition: the kernels get
    exactly them.  size: odd, in [3, 11]; sigma: finite and positive."""
    import numpy as np
    if isinstance(size, bool) or int(size) != size or not MIN_WINDOW <= int(size) <= MAX_WINDOW or int(size) % 2 == 0:
        raise ValueError("gaussian_window: size = %r, must be an odd integer in [%d, %d]" % (size, MIN_WINDOW, MAX_WINDOW))
    sigma = float(sigma)
    if not (0.0 < sigma < float("inf")):
        raise ValueError("gaussian_window: sigma = %r, must be finite and positive" % sigma)
    size = int(size)
    r = size // 2
    g = [_math.exp(-float((k - r) * (k - r)) / (2.0 * sigma * sigma)) for k in range(size)]
    total = sum(g)
    return np.array([v / total for v in g], dtype=np.float64).astype(np.float32)


class _Handle:
    """owner of a psdr_hip_ssim"""

    def __init__(self, width, height, channels, taps, c1, c2, padding, stream):
        from . import cabi
        self.ptr, self._cabi = _C.c_void_p(), cabi
        g = (_C.c_float * len(taps))(*[float(v) for v in taps])
        cabi.check(cabi.lib().psdr_hip_ssim_create(width, height, channels, len(taps), g, c1, c2, padding, _C.byref(self.ptr), stream))

    def __del__(self):
        if getattr(self, "ptr", None) and self._cabi is not None:
            self._cabi.lib().psdr_hip_ssim_destroy(self.ptr)
            self.ptr = None


@_functools.lru_cache(maxsize=None)
def _fn():
    import torch

    class _SSIMLossFn(torch.autograd.Function):
        """ss(img, target, mask): the forward also produces dloss / dimg, the backward scales it by the incoming scalar; target and mask get None"""

        @staticmethod
        def forward(ctx, ss, img, target, mask):
            out, grad = ss._eval(img, target, mask, True)
            ctx.save_for_backward(grad)
            ctx.like = (img.device, img.dtype)
            ss.ssim = out[1]
            return out[0]

        @staticmethod
        def backward(ctx, g):
            grad, = ctx.saved_tensors
            return None, (g * grad).to(*ctx.like) if ctx.needs_input_grad[1] else None, None, None

    return _SSIMLossFn


class SSIMLoss:
    """loss = 1 - mean SSIM of one frame size.

    width, height: the frame; channels: C in 1..4; window: K, odd in 3..11; sigma: of the Gaussian window; data_range, k1, k2: C1 = (k1 data_range)^2,
    C2 = (k2 data_range)^2; padding: "same" (every pixel counts, the window sees zeros outside the frame) or "valid" (only the pixels whose window lies wholly inside
    count; the frame must be at least window x window).

    ss(img, target, mask=None) takes [width * height, C] tensors (pixel p = y * width + x) and returns the loss as a 0-d float32 tensor on the render device, computed on
    torch's current stream without a host synchronisation.  It is differentiable in img only: target is detached - its gradient would need three more maps and nobody
    optimises a photograph - and so is mask ([W H] or [W H, 1], finite and non-negative); both get None.  The forward pass produces the gradient as well: backward only
    scales it.  ss.ssim holds the detached mean SSIM of the last call (0-d), ss.ssim_map() the unmasked per-pixel, per-channel S it saw.

    SSIM assumes a bounded range: tone-map HDR images into [0, data_range] before they get here.

    The handle owns work frames: calls on one SSIMLoss must follow each other on one stream."""

    def __init__(self, width, height, channels=3, window=11, sigma=1.5, data_range=1.0, k1=0.01, k2=0.03, padding="same"):
        import numpy as np
        width, height, channels = int(width), int(height), int(channels)
        if padding not in PADDINGS:
            raise ValueError("SSIMLoss: unknown padding %r (one of %s)" % (padding, ", ".join(sorted(PADDINGS))))
        if not 1 <= channels <= MAX_CHANNELS:
            raise ValueError("SSIMLoss: channels = %d, must lie in [1, %d]" % (channels, MAX_CHANNELS))
        if width < 1 or height < 1 or width > MAX_SIDE or height > MAX_SIDE or width * height > MAX_PIXELS:
            raise ValueError("SSIMLoss: a frame of %d x %d pixels; both sides must lie in [1, %d] and their product may be at most 2^24" % (width, height, MAX_SIDE))
        try:
            self.taps = gaussian_window(window, sigma)
        except ValueError as e:
            raise ValueError("SSIMLoss: " + str(e)) from None
        window = int(window)
        if padding == "valid" and (width < window or height < window):
            raise ValueError("SSIMLoss: padding=\"valid\" needs a frame of at least %d x %d pixels, got %d x %d" % (window, window, width, height))
        data_range, k1, k2 = float(data_range), float(k1), float(k2)
        c1, c2 = float(np.float32((k1 * data_range) ** 2)), float(np.float32((k2 * data_range) ** 2))
        if not (0.0 < c1 < float("inf") and 0.0 < c2 < float("inf")):
            raise ValueError("SSIMLoss: (k1 data_range)^2 = %r and (k2 data_range)^2 = %r must be finite and positive as float32 (data_range = %r, k1 = %r, k2 = %r)" %
                             (c1, c2, data_range, k1, k2))
        self.width, self.height, self.channels, self.window, self.sigma, self.padding = width, height, channels, window, float(sigma), padding
        self.data_range, self.k1, self.k2, self.c1, self.c2 = data_range, k1, k2, c1, c2
        self.ssim = None
        _single_gpu("SSIMLoss")
        from . import _device, _stream_ptr
        import torch
        self._device = _device()
        with torch.cuda.device(self._device):
            self._handle = _Handle(width, height, channels, self.taps, c1, c2, PADDINGS[padding], _stream_ptr())

    def _check_image(self, x, what):
        import torch
        n = self.width * self.height
        if not isinstance(x, torch.Tensor) or x.dim() != 2 or tuple(x.shape) != (n, self.channels) or not x.is_floating_point():
            raise ValueError("SSIMLoss: %s must be a floating-point [%d, %d] tensor, got %s" % (what, n, self.channels, tuple(x.shape) if hasattr(x, "shape") else type(x)))

    def _eval(self, img, target, mask, want_grad):
        """-> (out [2]: the loss and the mean SSIM, dloss / dimg [W H, C] or None), on the current stream"""
        import torch
        from . import cabi, _stream_ptr
        _single_gpu("SSIMLoss")
        n = self.width * self.height
        # every argument is looked at before the first one is moved to the device
        self._check_image(img, "img")
        self._check_image(target, "target")
        if mask is not None and (not isinstance(mask, torch.Tensor) or not mask.is_floating_point() or tuple(mask.shape) not in ((n,), (n, 1))):
            raise ValueError("SSIMLoss: mask must be a floating-point tensor of shape [%d] or [%d, 1], got %s" % (n, n, tuple(mask.shape) if hasattr(mask, "shape") else type(mask)))
        img, target, mask = (None if t is None else t.detach().to(self._device, torch.float32).contiguous() for t in (img, target, mask))
        with torch.cuda.device(self._device):
            out = torch.empty(2, device=self._device, dtype=torch.float32)
            grad = torch.empty_like(img) if want_grad else None
            cabi.check(cabi.lib().psdr_hip_ssim_eval(self._handle.ptr, img.data_ptr(), target.data_ptr(), mask.data_ptr() if mask is not None else None, out.data_ptr(),
                                                     grad.data_ptr() if want_grad else None, _stream_ptr()))
        return out, grad

    def __call__(self, img, target, mask=None):
        """the loss 1 - mean SSIM, a 0-d tensor"""
        return _fn().apply(self, img, target, mask)

    def value_and_grad(self, img, target, mask=None):
        """(loss, dloss / dimg) without autograd, both detached: what a hand-written adjoint needs"""
        out, grad = self._eval(img, target, mask, True)
        self.ssim = out[1]
        return out[0], grad

    def ssim_map(self):
        """the unmasked S [W H, C] of the last call, copied on the current stream"""
        import torch
        from . import cabi, _stream_ptr
        with torch.cuda.device(self._device):
            s = torch.empty((self.width * self.height, self.channels), device=self._device, dtype=torch.float32)
            cabi.check(cabi.lib().psdr_hip_ssim_map(self._handle.ptr, s.data_ptr(), _stream_ptr()))
        return s
