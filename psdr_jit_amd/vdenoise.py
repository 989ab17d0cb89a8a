"""Variance-guided a-trous denoiser that keeps illumination edges, with its frozen operator and that operator's transpose (kernels:
csrc/hip/vdenoise.hip).

psdr.Denoiser stops at edges of the first-hit guides only.  A shadow boundary, a caustic or a luminaire's penumbra on a flat surface has no guide edge, and five levels
wipe it out.  This filter adds the tap weight of Dammertz et al. 2010, normalised by variance as in SVGF (Schied et al. 2017): it falls off with the squared luminance
difference of the two pixels, measured in units of the variance of that difference - the per-pixel variance that render_c_sq / variance_from_sq already produce.

    img, sq = psdr.render_c_sq(integrator, sc, 0)
    var = psdr.luminance_variance(img, sq, sc.opts.spp)
    den = psdr.VarianceDenoiser(psdr.first_hit_guides(sc), sc.opts.width, sc.opts.height)        # levels=5, sigma_l=2
    out = den(img, var)                                                                          # den.variance: the filtered variance

The operator (include/psdr_hip.h states it in full).  The state is (x_l, v_l), x_0 = img, v_0 = var.  Level l = 0 .. L - 1, stride s = 2^l, taps (i, j) in {-2 .. 2}^2,
h = [1, 4, 6, 4, 1] / 16, exactly as in Denoiser:

    lum_l(p) = a_0 x_l,0(p) + a_1 x_l,1(p) + a_2 x_l,2(p)
    vt_l(p)  = 3 x 3 prefilter of v_l at unit stride, [1, 2, 1] x [1, 2, 1] / 16 over the taps inside the frame, divided by the sum of the coefficients that were inside
    q = p + s (i, j) exists only inside the frame;   d2 = sum_k (g_k(p) - g_k(q))^2;   z = k (lum_l(p) - lum_l(q))^2 / (vt_l(p) + vt_l(q) + eps),  k = 1 / sigma_l^2
    w_l(p, q) = h(i) h(j) exp(-(d2 + z)) if 0 <= d2 + z < inf and vt_l(p) + vt_l(q) + eps is finite, else 0;   the centre tap is h(0)^2 whatever the inputs hold;   a tap of weight 0 adds nothing
    N_l(p) = sum_q w_l(p, q);   x_{l+1}(p) = sum_q w_l(p, q) x_l(q) / N_l(p);   v_{l+1}(p) = sum_q w_l(p, q)^2 v_l(q) / N_l(p)^2

v_{l+1} is the exact variance of x_{l+1}'s luminance for one level with independent pixels and the weights held fixed; over several levels a level's inputs are
correlated, and it is SVGF's approximation.

The weights depend on the image, so the map is not linear.  A call records lum_l, vt_l and 1 / N_l; the recorded ("frozen") operator D_x is linear, den.frozen applies it to
any image and den.frozen_transpose applies its transpose, the same gather with the source pre-multiplied by 1 / N_l: no scatter, no atomics, the same bits every time.
The gradient autograd hands back through den(img, var) is D_x^T g: the EXACT TRANSPOSE OF THE FROZEN OPERATOR, the weights being constants (stop-gradient) - the usual
choice for a data-dependent filter inside a loss.  It is NOT the derivative of the nonlinear map, and var receives no gradient.

One GPU only: under an initialised torch.distributed group of more than one rank the calls raise."""
import ctypes as _C
import math as _math

import torch as _torch

from . import cabi as _cabi
from ._opcommon import _single_gpu
from .denoise import _Handle, _frame_guides

REC709 = (0.2126, 0.7152, 0.0722)


def _coefficients(what, luminance, channels):
    if luminance is None:
        return REC709 if channels == 3 else (1.0,)
    a = tuple(float(c) for c in luminance)
    if len(a) != channels or not all(_math.isfinite(c) for c in a):
        raise ValueError("%s: luminance = %r, expected %d finite coefficients" % (what, luminance, channels))
    return a


class _VDenoiseFn(_torch.autograd.Function):
    """den(img, var); backward is the transpose of the operator this call recorded, var gets None"""

    @staticmethod
    def forward(ctx, den, img, var):
        ctx.den, ctx.like = den, (img.device, img.dtype)
        out = den._apply(img, var)
        ctx.serial = den._serial
        return out

    @staticmethod
    def backward(ctx, g):
        if ctx.den._serial != ctx.serial:
            raise RuntimeError("VarianceDenoiser: a later call has replaced the record this backward needs; run backward() before the next den(img, var)")
        return None, ctx.den._frozen(g, True).to(*ctx.like), None


class VarianceDenoiser:
    """The variance-guided a-trous filter for one frame and one set of guides.

    guides: a [width * height, G] tensor, G <= 8, pre-scaled as for Denoiser (first_hit_guides does that), or None.  levels in 1..8.  sigma_l > 0: a tap's weight falls
    to e^-1 where the two luminances differ by sigma_l standard deviations of their difference; float('inf') gives k = 0, and the image part is then Denoiser's operator
    bit for bit.  eps > 0 guards the division where both variances are 0.  luminance: the coefficients a, default (0.2126, 0.7152, 0.0722) for 3 channels and (1) for one;
    given explicitly they fix the channel count.

    den(img, var): img float32 [width * height, C], C in {1, 3}; var [width * height] (or [.., 1]), the variance of the pixel's luminance estimate
    (luminance_variance).  On torch's current stream, two launches per level.  It records the weights; den.variance is v_L of the last call, detached.
    den.frozen(u) = D_x u and den.frozen_transpose(y) = D_x^T y use the last call's record (C of u, y need not be the recording's); before a first call they raise.
    den(img, var) is differentiable in img with backward = den.frozen_transpose: the transpose of the frozen operator, not the derivative of the nonlinear map; var gets no
    gradient.  The forward derivative of a denoised image under the same convention is den.frozen(psdr.forward_grad(img, P)).

    The handle owns the record (12 levels width height bytes: 252 MB at 2048 x 2048, 5 levels) and the work frames: calls on one VarianceDenoiser must follow each other
    on one stream, and a backward must run before the next den(img, var)."""

    def __init__(self, guides, width, height, levels=5, sigma_l=2.0, eps=1e-12, luminance=None):
        from . import _stream_ptr
        width, height, levels = int(width), int(height), int(levels)
        sigma_l, eps = float(sigma_l), float(eps)
        if not sigma_l > 0.0:
            raise ValueError("VarianceDenoiser: sigma_l = %r, must be positive (float('inf') switches the luminance weight off)" % sigma_l)
        if not (eps > 0.0 and _math.isfinite(eps)):
            raise ValueError("VarianceDenoiser: eps = %r, must be positive and finite" % eps)
        if luminance is not None:
            luminance = tuple(float(c) for c in luminance)
            if len(luminance) not in (1, 3) or not all(_math.isfinite(c) for c in luminance):
                raise ValueError("VarianceDenoiser: luminance = %r, expected 1 or 3 finite coefficients" % (luminance,))
        self._device, g, self.n_guides = _frame_guides("VarianceDenoiser", guides, width, height, levels)
        self.width, self.height, self.levels = width, height, levels
        self.sigma_l, self.eps, self.luminance = sigma_l, eps, luminance
        self.k = 0.0 if _math.isinf(sigma_l) else 1.0 / (sigma_l * sigma_l)
        self.variance = None
        self._serial = 0
        with _torch.cuda.device(self._device):
            self._handle = _Handle("psdr_hip_vdenoise", g, self.n_guides, width, height, levels, _stream_ptr())

    def _image(self, x):
        n = self.width * self.height
        if x.dim() != 2 or int(x.shape[0]) != n or int(x.shape[1]) not in (1, 3):
            raise ValueError("VarianceDenoiser: expected a [%d, C] tensor with C in {1, 3}, got %s" % (n, tuple(x.shape)))
        return x.detach().to(self._device, _torch.float32).contiguous()

    def _apply(self, img, var):
        from . import _stream_ptr
        _single_gpu("VarianceDenoiser")
        n = self.width * self.height
        if var.dim() not in (1, 2) or int(var.shape[0]) != n or (var.dim() == 2 and int(var.shape[1]) != 1):
            raise ValueError("VarianceDenoiser: expected a variance of shape [%d] or [%d, 1], got %s" % (n, n, tuple(var.shape)))
        x = self._image(img)
        C = int(x.shape[1])
        a = _coefficients("VarianceDenoiser", self.luminance, C)
        v = var.detach().to(self._device, _torch.float32).reshape(n).contiguous()
        out, v_out = _torch.empty_like(x), _torch.empty_like(v)
        self._serial += 1
        _cabi.check(_cabi.lib().psdr_hip_vdenoise_apply(self._handle.ptr, x.data_ptr(), C, v.data_ptr(), (_C.c_float * C)(*a), self.k, self.eps, out.data_ptr(), v_out.data_ptr(),
                                                       _stream_ptr()))
        self.variance = v_out
        return out

    def _frozen(self, u, adjoint):
        from . import _stream_ptr
        _single_gpu("VarianceDenoiser")
        u = self._image(u)
        if not self._serial:
            raise RuntimeError("VarianceDenoiser: no record yet: den(img, var) makes one")
        out = _torch.empty_like(u)
        L = _cabi.lib()
        call = L.psdr_hip_vdenoise_frozen_adj if adjoint else L.psdr_hip_vdenoise_frozen
        _cabi.check(call(self._handle.ptr, u.data_ptr(), int(u.shape[1]), out.data_ptr(), _stream_ptr()))
        return out

    def __call__(self, img, var):
        """x_L; records the weights"""
        return _VDenoiseFn.apply(self, img, var)

    def frozen(self, u):
        """D_x u with the last call's record (detached)"""
        return self._frozen(u, False)

    def frozen_transpose(self, y):
        """D_x^T y with the last call's record (detached)"""
        return self._frozen(y, True)

    def record(self):
        """the last call's record, float32 [levels, 3, width * height]: lum_l, vt_l, 1 / N_l (a copy)"""
        from . import _stream_ptr
        if not self._serial:
            raise RuntimeError("VarianceDenoiser: no record yet: den(img, var) makes one")
        out = _torch.empty((self.levels, 3, self.width * self.height), device=self._device, dtype=_torch.float32)
        _cabi.check(_cabi.lib().psdr_hip_vdenoise_record(self._handle.ptr, out.data_ptr(), _stream_ptr()))
        return out


def luminance_variance(mean, sq, n, luminance=None):
    """The variance of a pixel's luminance estimate from render_c_sq's outputs: (sum_c a_c sqrt(max(variance_from_sq(mean, sq, n)_c, 0)))^2, float32 [n_pixels].

    The channels of one path sample are nearly perfectly correlated (a path's throughput scales all three), and this is the variance of sum_c a_c x_c under perfect
    correlation: the standard deviations add.  luminance: the coefficients a, default (0.2126, 0.7152, 0.0722) for 3 channels and (1) for one."""
    from . import variance_from_sq
    var = variance_from_sq(mean, sq, n)
    if var.dim() != 2 or int(var.shape[1]) not in (1, 3):
        raise ValueError("luminance_variance: expected [n_pixels, C] tensors with C in {1, 3}, got %s" % (tuple(var.shape),))
    a = _coefficients("luminance_variance", luminance, int(var.shape[1]))
    sd = var.clamp_min(0).sqrt() * _torch.tensor(a, device=var.device, dtype=var.dtype)
    return sd.sum(dim=1) ** 2
