"""Edge-avoiding a-trous denoiser guided by first-hit fields, with its transpose (kernels: csrc/hip/denoise.hip).

A path-traced frame keeps noise that no sample placement removes; a wavelet filter whose taps stop at the edges of noise-free guide images (Dammertz et al.
2010, "Edge-Avoiding A-Trous Wavelet Transform for fast Global Illumination Filtering") removes most of it.  The guides are what FieldExtractionIntegrator
renders: normals, positions, the silhouette, the BSDF value at the first hit, in the frame's own pixel order.

    guides = psdr.first_hit_guides(sc)                                   # [W H, G], scaled so that the weight of a tap is exp(-|difference|^2)
    den = psdr.Denoiser(guides, sc.opts.width, sc.opts.height)           # levels=5: a 125 x 125 pixel footprint
    loss(den(integrator.renderD(sc, 0))).backward()                      # or den(img) on a final frame

The operator (include/psdr_hip.h states it in full): level l = 0 .. L - 1 averages the 5 x 5 taps q = p + 2^l (i, j) that lie inside the frame with the weights
h(i) h(j) exp(-sum_k (g_k(p) - g_k(q))^2), h = [1, 4, 6, 4, 1] / 16 (0 where that sum is not finite; the centre tap keeps h(0)^2 whatever the guides hold), divided
by their sum.  The filter is linear in the image and every level is an average: it never leaves the range of its input.  Its transpose is the same gather with
the source divided by the sums beforehand, so neither direction scatters or uses an atomic: two calls give the same bits.

One GPU only: under an initialised torch.distributed group of more than one rank the calls raise."""
import ctypes as _C

import torch as _torch

from . import cabi as _cabi
from ._opcommon import _single_gpu

MAX_GUIDES, MAX_CHANNELS, MAX_LEVELS, MAX_PIXELS = 8, 4, 8, 1 << 24

FIELD_CHANNELS = {"silhouette": 1, "position": 3, "depth": 1, "geoNormal": 3, "shNormal": 3, "uv": 2, "bsdf": 3}          # what a field contributes to the guides
DEFAULT_SIGMA = {"silhouette": 0.1, "shNormal": 0.25, "geoNormal": 0.25, "bsdf": 0.1}                                      # position, depth, uv: relative, see first_hit_guides
RELATIVE_SIGMA = 0.05


class _Handle:
    """owner of a psdr_hip_denoise or a psdr_hip_vdenoise: `prefix` + "_create" / "_destroy" are its entry points"""

    def __init__(self, prefix, guides, n_guides, width, height, levels, stream):
        self.ptr, self._destroy = _C.c_void_p(), prefix + "_destroy"
        _cabi.check(getattr(_cabi.lib(), prefix + "_create")(guides.data_ptr() if guides is not None else None, n_guides, width, height, levels, _C.byref(self.ptr), stream))

    def __del__(self):
        if getattr(self, "ptr", None) and _cabi is not None:           # (None: the interpreter is shutting down and has cleared the module)
            getattr(_cabi.lib(), self._destroy)(self.ptr)
            self.ptr = None


def _frame_guides(what, guides, width, height, levels):
    """What the constructor of `what` (the class, for the messages) does with its frame, levels and guides: it refuses wrong ones, then a process group of several ranks,
    and only then touches the device -> (device, the guides detached, in float32 and contiguous on it, or None without guides, their channel count)"""
    from . import _device
    if width < 1 or height < 1 or width * height > MAX_PIXELS:
        raise ValueError("%s: a frame of %d x %d pixels; both must be positive and their product at most 2^24" % (what, width, height))
    if not 1 <= levels <= MAX_LEVELS:
        raise ValueError("%s: levels = %d, must lie in [1, %d]" % (what, levels, MAX_LEVELS))
    if guides is not None:
        if guides.dim() != 2 or int(guides.shape[0]) != width * height:
            raise ValueError("%s: expected guides of shape [%d, G], got %s" % (what, width * height, tuple(guides.shape)))
        if int(guides.shape[1]) > MAX_GUIDES:
            raise ValueError("%s: %d guide channels, at most %d" % (what, int(guides.shape[1]), MAX_GUIDES))
    _single_gpu(what)
    n_guides = int(guides.shape[1]) if guides is not None else 0
    device = _device()
    return device, (guides.detach().to(device, _torch.float32).contiguous() if n_guides else None), n_guides


class _DenoiseFn(_torch.autograd.Function):
    """den(img); the filter is linear, so the backward is its transpose"""

    @staticmethod
    def forward(ctx, den, img):
        ctx.den, ctx.like = den, (img.device, img.dtype)
        return den._run(img, False)

    @staticmethod
    def backward(ctx, g):
        return None, ctx.den._run(g, True).to(*ctx.like)


class Denoiser:
    """D = A_{L-1} ... A_0 for one frame and one set of guides.

    guides: a [width * height, G] tensor, G <= 8, pixel p = y * width + x, already scaled (first_hit_guides does that: the weight of a tap is
    exp(-sum_k (g_k(p) - g_k(q))^2)); or None, which gives the plain B3-spline a-trous smoother.  The guides are detached and copied: they carry no gradient,
    and the normalisers 1 / N_l are computed from them once, here.  levels in 1..8; level l reaches 2 * 2^l pixels to each side.

    den(img) applies D to a float32 [width * height, C] tensor, C <= 4, on torch's current stream, one launch per level; it is differentiable in img, the backward
    being den.transpose.  den.transpose(y) = D^T y is public: it is what a hand-written adjoint needs.

    D is linear, so the forward derivative of a denoised image is the denoised forward derivative: den(psdr.forward_grad(img, P)).

    The handle owns two work frames: calls on one Denoiser must follow each other on one stream."""

    def __init__(self, guides, width, height, levels=5):
        from . import _stream_ptr
        width, height, levels = int(width), int(height), int(levels)
        self._device, g, self.n_guides = _frame_guides("Denoiser", guides, width, height, levels)
        self.width, self.height, self.levels = width, height, levels
        with _torch.cuda.device(self._device):
            self._handle = _Handle("psdr_hip_denoise", g, self.n_guides, width, height, levels, _stream_ptr())

    def _run(self, x, adjoint):
        from . import _stream_ptr
        _single_gpu("Denoiser")
        n = self.width * self.height
        if x.dim() != 2 or int(x.shape[0]) != n or not 1 <= int(x.shape[1]) <= MAX_CHANNELS:
            raise ValueError("Denoiser: expected a [%d, C] tensor with C in 1..%d, got %s" % (n, MAX_CHANNELS, tuple(x.shape)))
        x = x.detach().to(self._device, _torch.float32).contiguous()
        out = _torch.empty_like(x)
        L = _cabi.lib()
        call = L.psdr_hip_denoise_apply_adj if adjoint else L.psdr_hip_denoise_apply
        _cabi.check(call(self._handle.ptr, x.data_ptr(), int(x.shape[1]), out.data_ptr(), _stream_ptr()))
        return out

    def __call__(self, img):
        """D img"""
        return _DenoiseFn.apply(self, img)

    def transpose(self, y):
        """D^T y (detached)"""
        return self._run(y, True)


def first_hit_guides(scene, sensor_id=0, seed=-1, fields=("silhouette", "shNormal", "position"), sigma=None):
    """The guides of a Denoiser from the scene's noise-free first-hit fields: float32 [n_pixels, G], detached.

    Every field of `fields` is rendered with FieldExtractionIntegrator(field).renderC(scene, sensor_id, seed) and divided by sigma sqrt(2), so that a tap's weight is
    exp(-|difference of the field|^2 / (2 sigma^2)); the channels are concatenated in the order of `fields`.  silhouette and depth contribute one channel, uv two,
    position, geoNormal, shNormal and bsdf three; more than 8 channels in all are refused (before anything is rendered).  The default set has 7; "bsdf" in place of
    "position" keeps texture detail on flat surfaces.

    sigma: a dict field -> float that overrides the defaults
        silhouette 0.1, shNormal and geoNormal 0.25 (unit vectors: a 20 degree turn weighs e^-1), bsdf 0.1,
        position, depth, uv: 0.05 x the largest extent of the field's values over the pixels that hit something (the largest of the per-channel max - min; 1 where
        nothing is hit), computed with torch ops on the device, without a host copy.
    These defaults are starting points chosen by reasoning about the fields' ranges.  They have not been measured against a quality metric."""
    from . import FieldExtractionIntegrator
    fields = tuple(fields)
    if not fields:
        raise ValueError("first_hit_guides: no field given (Denoiser(None, ...) is the filter without guides)")
    for f in fields:
        if f not in FIELD_CHANNELS:
            raise ValueError("first_hit_guides: unknown field %r, known: %s" % (f, ", ".join(sorted(FIELD_CHANNELS))))
    total = sum(FIELD_CHANNELS[f] for f in fields)
    if total > MAX_GUIDES:
        raise ValueError("first_hit_guides: fields %s add up to %d channels, at most %d" % (fields, total, MAX_GUIDES))
    sigma = dict(sigma or {})
    for f, v in sigma.items():
        if f not in fields or not float(v) > 0.0:
            raise ValueError("first_hit_guides: sigma[%r] = %r; a key must be one of the fields and its value positive" % (f, v))
    _single_gpu("first_hit_guides")
    hit = None
    parts = []
    for f in fields:
        img = FieldExtractionIntegrator(f).renderC(scene, sensor_id, seed)[:, :FIELD_CHANNELS[f]]
        if f in sigma:
            s = float(sigma[f])
        elif f in DEFAULT_SIGMA:
            s = DEFAULT_SIGMA[f]
        else:
            if hit is None:
                hit = FieldExtractionIntegrator("silhouette").renderC(scene, sensor_id, seed)[:, :1] > 0
            big = _torch.finfo(img.dtype).max
            extent = (_torch.where(hit, img, -big).amax(dim=0) - _torch.where(hit, img, big).amin(dim=0)).amax()
            s = RELATIVE_SIGMA * _torch.where(extent > 0, extent, _torch.ones_like(extent))          # (no pixel hit: -big - big < 0)
        parts.append(img / (s * 2.0 ** 0.5))
    return _torch.cat(parts, dim=1).contiguous()
