"""The multi-scale image loss: a sum of per-level losses over an image pyramid of the residual, value and gradient in one fused pass (DESIGN.md section 7h;
kernels: csrc/hip/msloss.hip).

A per-pixel loss carries no signal once a silhouette is more than a pixel from its target; the coarse levels of a pyramid carry it across the frame.  It is the
image-side counterpart of starting on a coarse mesh.

    ms = psdr.MultiScaleLoss(sc.opts.width, sc.opts.height)              # channels=3, every level down to 1 x 1, norm="l1"
    ms(den(integrator.renderD(sc, 0)), target).backward()                # or ms(img, target, weight=mask)

The definition (include/psdr_hip.h states it in full).  img, target [W H, C], pixel (x, y) at row y W + x; weight absent, [W H], [W H, 1] or [W H, C], without gradient.
d_0 = weight (img - target); level l + 1 has ceil(W_l / 2) x ceil(H_l / 2) pixels, each the mean of those of its 2 x 2 pixels of d_l that exist (this is
F.avg_pool2d(x, 2, ceil_mode=True, count_include_pad=False)); level_loss_l = sum rho(d_l) / (C W_l H_l) with rho = |x| ("l1", rho'(0) = 0) or x^2 ("l2");
loss = sum_l lambda_l level_loss_l.  Three launches give the loss, the level losses and dloss / dimg; no atomics: the same input gives the same bits.

One GPU only: under an initialised torch.distributed group of more than one rank the calls raise."""
import ctypes as _C
import functools as _functools

from ._opcommon import _single_gpu

NORMS = {"l1": 0, "l2": 1}          # PSDR_MSLOSS_L1, PSDR_MSLOSS_L2
MAX_CHANNELS, MAX_SIDE, MAX_PIXELS = 4, 16384, 1 << 24


def pyramid_shapes(width, height, levels=None):
    """[(W_l, H_l)] of levels l = 0 .. L - 1: each level halves both sides, rounding up.  levels=None: down to the 1 x 1 level; more than that is a ValueError."""
    width, height = int(width), int(height)
    if width < 1 or height < 1:
        raise ValueError("pyramid_shapes: a frame of %d x %d pixels; both must be positive" % (width, height))
    shapes = [(width, height)]
    while shapes[-1] != (1, 1):
        w, h = shapes[-1]
        shapes.append(((w + 1) // 2, (h + 1) // 2))
    if levels is None:
        return shapes
    if int(levels) != levels or not 1 <= int(levels) <= len(shapes):
        raise ValueError("pyramid_shapes: levels = %r, must be an integer in [1, %d] for %d x %d" % (levels, len(shapes), width, height))
    return shapes[:int(levels)]


class _Handle:
    """owner of a psdr_hip_msloss"""

    def __init__(self, width, height, levels, channels, stream):
        from . import cabi
        self.ptr, self._cabi = _C.c_void_p(), cabi
        cabi.check(cabi.lib().psdr_hip_msloss_create(width, height, levels, channels, _C.byref(self.ptr), stream))

    def __del__(self):
        if getattr(self, "ptr", None) and self._cabi is not None:
            self._cabi.lib().psdr_hip_msloss_destroy(self.ptr)
            self.ptr = None


@_functools.lru_cache(maxsize=None)
def _fn():
    import torch

    class _MultiScaleLossFn(torch.autograd.Function):
        """ms(img, target, weight): the forward also produces dloss / dimg, the backward scales it by the incoming scalar"""

        @staticmethod
        def forward(ctx, ms, img, target, weight):
            out, grad = ms._eval(img, target, weight, True)
            ctx.save_for_backward(grad)
            ctx.like = [(t.device, t.dtype) for t in (img, target)]
            ms.level_losses = out[1:]
            return out[0]

        @staticmethod
        def backward(ctx, g):
            grad, = ctx.saved_tensors
            gi = g * grad
            return (None, gi.to(*ctx.like[0]) if ctx.needs_input_grad[1] else None, (-gi).to(*ctx.like[1]) if ctx.needs_input_grad[2] else None, None)

    return _MultiScaleLossFn


class MultiScaleLoss:
    """loss = sum_l lambda_l mean(rho(d_l)) over the residual pyramid of one frame size.

    width, height: the frame; channels: C in 1..4; levels: L, None = every level down to 1 x 1 (pyramid_shapes); norm: "l1" or "l2"; level_weights: L numbers
    lambda_l, None = all 1.

    ms(img, target, weight=None) takes [width * height, C] tensors (pixel p = y * width + x) and returns the loss as a 0-d float32 tensor on the render device, computed
    on torch's current stream without a host synchronisation.  It is differentiable in img and target (the target's gradient is the negated image gradient); weight
    ([W H], [W H, 1] or [W H, C]: a mask, or 1 / sqrt(var + eps) from render_c_sq) is detached and gets none.  The forward pass produces the gradient as well: backward
    only scales it.  ms.level_losses holds the detached per-level losses [L] of the last call, ms.residual_pyramid() the d_l it saw.

    The handle owns work frames: calls on one MultiScaleLoss must follow each other on one stream."""

    def __init__(self, width, height, channels=3, levels=None, norm="l1", level_weights=None):
        width, height, channels = int(width), int(height), int(channels)
        if norm not in NORMS:
            raise ValueError("MultiScaleLoss: unknown norm %r (one of %s)" % (norm, ", ".join(sorted(NORMS))))
        if not 1 <= channels <= MAX_CHANNELS:
            raise ValueError("MultiScaleLoss: channels = %d, must lie in [1, %d]" % (channels, MAX_CHANNELS))
        if width < 1 or height < 1 or width > MAX_SIDE or height > MAX_SIDE or width * height > MAX_PIXELS:
            raise ValueError("MultiScaleLoss: a frame of %d x %d pixels; both sides must lie in [1, %d] and their product may be at most 2^24" % (width, height, MAX_SIDE))
        self.shapes = pyramid_shapes(width, height, levels)
        self.width, self.height, self.channels, self.levels, self.norm = width, height, channels, len(self.shapes), norm
        if level_weights is None:
            level_weights = [1.0] * self.levels
        level_weights = [float(v) for v in level_weights]
        if len(level_weights) != self.levels or not all(abs(v) < float("inf") for v in level_weights):
            raise ValueError("MultiScaleLoss: level_weights must be %d finite numbers, got %r" % (self.levels, level_weights))
        self.level_weights = tuple(level_weights)
        self._lambda = (_C.c_float * self.levels)(*level_weights)
        self.level_losses = None
        _single_gpu("MultiScaleLoss")
        from . import _device, _stream_ptr
        import torch
        self._device = _device()
        with torch.cuda.device(self._device):
            self._handle = _Handle(width, height, self.levels, channels, _stream_ptr())

    def _image(self, x, what):
        import torch
        n = self.width * self.height
        if not isinstance(x, torch.Tensor) or x.dim() != 2 or tuple(x.shape) != (n, self.channels) or not x.is_floating_point():
            raise ValueError("MultiScaleLoss: %s must be a floating-point [%d, %d] tensor, got %s" % (what, n, self.channels, tuple(x.shape) if hasattr(x, "shape") else type(x)))
        return x.detach().to(self._device, torch.float32).contiguous()

    def _eval(self, img, target, weight, want_grad):
        """-> (out [1 + L]: the loss and the level losses, dloss / dimg [W H, C] or None), on the current stream"""
        import torch
        from . import cabi, _stream_ptr
        _single_gpu("MultiScaleLoss")
        n = self.width * self.height
        img, target = self._image(img, "img"), self._image(target, "target")
        wc = 0
        if weight is not None:
            if not isinstance(weight, torch.Tensor) or not weight.is_floating_point() or tuple(weight.shape) not in ((n,), (n, 1), (n, self.channels)):
                raise ValueError("MultiScaleLoss: weight must be a floating-point tensor of shape [%d], [%d, 1] or [%d, %d], got %s" %
                                 (n, n, n, self.channels, tuple(weight.shape) if hasattr(weight, "shape") else type(weight)))
            wc = 1 if weight.dim() == 1 else int(weight.shape[1])
            weight = weight.detach().to(self._device, torch.float32).contiguous()
        with torch.cuda.device(self._device):
            out = torch.empty(1 + self.levels, device=self._device, dtype=torch.float32)
            grad = torch.empty_like(img) if want_grad else None
            cabi.check(cabi.lib().psdr_hip_msloss_eval(self._handle.ptr, img.data_ptr(), target.data_ptr(), weight.data_ptr() if wc else None, wc, NORMS[self.norm],
                                                       self._lambda, out.data_ptr(), grad.data_ptr() if want_grad else None, _stream_ptr()))
        return out, grad

    def __call__(self, img, target, weight=None):
        """the loss, a 0-d tensor"""
        return _fn().apply(self, img, target, weight)

    def value_and_grad(self, img, target, weight=None):
        """(loss, dloss / dimg) without autograd, both detached: what a hand-written adjoint needs"""
        out, grad = self._eval(img, target, weight, True)
        self.level_losses = out[1:]
        return out[0], grad

    def residual_pyramid(self):
        """[d_l as a [W_l * H_l, C] tensor] of the last call, copied on the current stream"""
        import torch
        from . import cabi, _stream_ptr
        levels = []
        with torch.cuda.device(self._device):
            for l, (w, h) in enumerate(self.shapes):
                d = torch.empty((w * h, self.channels), device=self._device, dtype=torch.float32)
                cabi.check(cabi.lib().psdr_hip_msloss_level(self._handle.ptr, l, d.data_ptr(), _stream_ptr()))
                levels.append(d)
        return levels
