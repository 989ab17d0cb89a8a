"""Regularisers of a signed distance on a lattice - Eikonal, Laplacian, sign-change cross-entropy - with their gradient in one fused stencil (kernels:
csrc/hip/latreg.hip).

`MarchingTetrahedra` hands a gradient to the two ends of a crossing lattice edge only; nothing else constrains the rest of the field.  These are the three terms every DMTet /
nvdiffrec-style loop adds for that, what `MeshRegularizer` is to a fixed topology:

    lr   = psdr.LatticeRegularizer((nx, ny, nz), spacing, weights=(1.0, 0.0, 0.0), sign_scale=1.0)      # spacing: a number or three
    h    = psdr.lattice_spacing((nx, ny, nz), lo, hi)      # (hi - lo) / (n - 1) in float64, the spacing of psdr.lattice_points
    loss = lr(sdf)                                         # a scalar on the render device, differentiable in sdf; backward only scales the stored gradient
    lr.terms, lr.num_crossings                             # float32 [3] and int32 [1] device tensors of the last call, detached; reading them is the caller's synchronisation
    loss, grad = lr.value_and_grad(sdf)                    # without autograd, the same bits

The definition is stated once, in include/psdr_hip.h (THE LATTICE REGULARISERS).  In outline, on marching tetrahedra's lattice (u = x + nx (y + ny z), inside where sdf < 0):

    eikonal   = (1 / Nc) sum_cells (n - 1)^2, n the length of the means of the cell's four edge differences along each axis over the spacing; a cell with n = 0 adds 1, no gradient
    laplacian = (1 / Nv) sum_u r_u^2, r_u = sum_a ((s_- - s_u) + (s_+ - s_u)) / h_a^2 over the axes along which u has both neighbours: a linear field gives exactly 0
    sign      = (1 / V) sum over the crossing edges (a, b) of the seven classes of bce(k s_a, y_b) + bce(k s_b, y_a) = (1 / V) sum_u m_u softplus(k |s_u|); V, the number of
                crossing edges, is held constant in the gradient, and V = 0 gives 0
    loss      = w_eik eikonal + w_lap laplacian + w_sign sign; a term of weight 0 is not evaluated and reports 0 (num_crossings is 0 where w_sign is)

sdf is expected to be finite: nothing checks it (a check would synchronise); a NaN gives NaNs, never an access out of range.  One GPU only: under an initialised
torch.distributed group of more than one rank the calls raise."""
import collections as _collections
import ctypes as _C
import functools as _functools
import math as _math

import numpy as _np

from ._opcommon import _as_tensor, _ceil_div, _checked_shape, _single_gpu

TILE = (32, 8, 4)          # the vertices of a workgroup's tile (csrc/hip/latreg.hip: kTX, kTY, kTZ)

LatregPlan = _collections.namedtuple("LatregPlan", ["tile", "num_lattice", "num_cells", "workgroups", "scratch_floats"])


def launch_plan_lr(shape):
    """How the passes over a lattice of `shape` are split: LatregPlan(tile = (tx, ty, tz), num_lattice, num_cells, workgroups, scratch_floats), a pure function
    (csrc/hip/latreg.hip: psdr_hip_latreg_plan gives the same numbers).  A workgroup owns a tile of tx x ty x tz vertices, loaded once into LDS with its halo; there are
    ceil(nx / tx) ceil(ny / ty) ceil(nz / tz) of them, each with four partial sums in `scratch`."""
    nx, ny, nz = _checked_shape(shape, "launch_plan_lr")
    wg = _ceil_div(nx, TILE[0]) * _ceil_div(ny, TILE[1]) * _ceil_div(nz, TILE[2])
    return LatregPlan(TILE, nx * ny * nz, (nx - 1) * (ny - 1) * (nz - 1), wg, 4 * wg)


def _three(q, what, name):
    import torch
    try:
        return _np.broadcast_to(_np.asarray(q.detach().cpu().numpy() if isinstance(q, torch.Tensor) else q, dtype=_np.float64), (3,))
    except (TypeError, ValueError):
        raise ValueError("%s: %s must be a number or three numbers, got %r" % (what, name, q)) from None


def lattice_spacing(shape, lo=-1.0, hi=1.0):
    """The spacing of psdr.lattice_points(shape, lo, hi): (hi - lo) / (n - 1) per axis, a tuple of three floats evaluated in float64.  lo, hi: numbers or three numbers
    each, hi > lo in every component."""
    n = _checked_shape(shape, "lattice_spacing")
    lo3, hi3 = _three(lo, "lattice_spacing", "lo"), _three(hi, "lattice_spacing", "hi")
    if not (_np.isfinite(lo3).all() and _np.isfinite(hi3).all() and (hi3 > lo3).all()):
        raise ValueError("lattice_spacing: lo and hi must be finite with hi > lo in every component, got %r and %r" % (lo, hi))
    return tuple(float((hi3[a] - lo3[a]) / (n[a] - 1)) for a in range(3))


def _checked_spacing(spacing):
    h = _three(spacing, "LatticeRegularizer", "spacing")
    if not (_np.isfinite(h).all() and (h > 0).all()):
        raise ValueError("LatticeRegularizer: spacing must be finite and positive, got %r" % (spacing,))
    with _np.errstate(over="ignore", under="ignore", divide="ignore"):
        recip = _np.concatenate([1.0 / (4.0 * h), 1.0 / (h * h)]).astype(_np.float32)
    if not (_np.isfinite(recip).all() and (recip > 0).all()):
        raise ValueError("LatticeRegularizer: spacing = %r: 1 / (4 h) and 1 / h^2 must be positive float32 numbers" % (spacing,))
    return tuple(float(x) for x in h)


def _checked_weights(weights):
    try:
        w = tuple(float(x) for x in weights)
    except (TypeError, ValueError):
        raise ValueError("LatticeRegularizer: weights must be three numbers (eikonal, laplacian, sign), got %r" % (weights,)) from None
    if len(w) != 3 or not all(_math.isfinite(x) and x >= 0.0 for x in w):
        raise ValueError("LatticeRegularizer: weights must be three finite numbers >= 0 (eikonal, laplacian, sign), got %r" % (weights,))
    return w


def _checked_scale(sign_scale):
    try:
        k = float(sign_scale)
    except (TypeError, ValueError):
        raise ValueError("LatticeRegularizer: sign_scale must be a number, got %r" % (sign_scale,)) from None
    if not (_math.isfinite(k) and k >= 0.0):
        raise ValueError("LatticeRegularizer: sign_scale = %r, must be finite and >= 0" % (sign_scale,))
    return k


@_functools.lru_cache(maxsize=None)
def _fn():
    import torch

    class _LatRegFn(torch.autograd.Function):
        """lr(sdf): the forward also produces dloss / dsdf, the backward scales it by the incoming scalar"""

        @staticmethod
        def forward(ctx, lr, sdf):
            out, crossings, grad = lr._eval(sdf, True)
            ctx.save_for_backward(grad)
            ctx.like = (sdf.device, sdf.dtype)
            lr.terms, lr.num_crossings = out[1:], crossings
            return out[0]

        @staticmethod
        def backward(ctx, g):
            grad, = ctx.saved_tensors
            return None, (g * grad).to(*ctx.like)

    return _LatRegFn


class LatticeRegularizer:
    """loss = w_eik eikonal + w_lap laplacian + w_sign sign of a signed distance on a regular lattice of `shape` = (nx, ny, nz) vertices (the module's docstring outlines the
    definition, include/psdr_hip.h states it).

    spacing: a number or three, finite and positive (psdr.lattice_spacing gives that of psdr.lattice_points).  weights = (w_eik, w_lap, w_sign), finite and >= 0;
    sign_scale >= 0 multiplies sdf inside the sign term's cross-entropy.  weights and sign_scale are plain attributes read at every call, so a schedule can change them; a
    term whose weight is 0 is not evaluated and reports 0.

    lr(sdf) takes a [Nv] tensor on any device and of any float dtype and returns the loss as a 0-d float32 tensor on the render device, computed on torch's current stream
    without a host synchronisation.  It is differentiable in sdf: the forward pass produces the gradient as well, backward only scales it, and the gradient returns to sdf's
    device and dtype.  lr.value_and_grad(sdf) returns (loss, dloss / dsdf) detached, the same bits; lr.value(sdf) is the value-only call (no gradient pass).  lr.terms holds
    the detached float32 [3] tensor (eikonal, laplacian, sign) and lr.num_crossings the int32 [1] tensor V of the last call, both on the device.  Every call allocates its
    own work arrays: calls may be in flight on several streams."""

    def __init__(self, shape, spacing, weights=(1.0, 0.0, 0.0), sign_scale=1.0):
        # every argument is checked before a device is looked for
        self.shape = _checked_shape(shape, "LatticeRegularizer")
        self.spacing = _checked_spacing(spacing)
        self.weights, self.sign_scale = _checked_weights(weights), _checked_scale(sign_scale)
        self.num_lattice = self.shape[0] * self.shape[1] * self.shape[2]
        self.terms = None
        self.num_crossings = None

    def _checked_sdf(self, sdf):
        sdf = _as_tensor(sdf)
        if tuple(sdf.shape) != (self.num_lattice,) or not sdf.is_floating_point():
            raise ValueError("LatticeRegularizer: sdf must be a floating-point [%d] tensor (shape %r), got %s %s" % (self.num_lattice, self.shape, sdf.dtype, tuple(sdf.shape)))
        return sdf

    def _eval(self, sdf, want_grad):
        """-> (out [4]: the loss and the three terms, crossings int32 [1], dloss / dsdf [Nv] or None), on the current stream"""
        import torch
        sdf = self._checked_sdf(sdf)
        w, k = _checked_weights(self.weights), _checked_scale(self.sign_scale)
        _single_gpu("LatticeRegularizer")
        from . import cabi, _device, _stream_ptr
        device = _device()
        nx, ny, nz = self.shape
        plan = launch_plan_lr(self.shape)
        with torch.cuda.device(device):
            s = sdf.detach().to(device, torch.float32).contiguous()
            scratch = torch.empty(plan.scratch_floats, device=device, dtype=torch.float32)
            out = torch.empty(4, device=device, dtype=torch.float32)
            crossings = torch.empty(1, device=device, dtype=torch.int32)
            grad = torch.empty_like(s) if want_grad else None
            cabi.check(cabi.lib().psdr_hip_latreg_eval(s.data_ptr(), nx, ny, nz, (_C.c_double * 3)(*self.spacing), (_C.c_float * 3)(*w), k, scratch.data_ptr(), out.data_ptr(),
                                                       crossings.data_ptr(), grad.data_ptr() if want_grad else None, _stream_ptr()))
        return out, crossings, grad

    def __call__(self, sdf):
        """the loss, a 0-d tensor"""
        return _fn().apply(self, self._checked_sdf(sdf))

    def value_and_grad(self, sdf):
        """(loss, dloss / dsdf) without autograd, both detached on the render device: what a hand-written adjoint needs"""
        out, crossings, grad = self._eval(sdf, True)
        self.terms, self.num_crossings = out[1:], crossings
        return out[0], grad

    def value(self, sdf):
        """the loss alone, detached: two launches instead of three"""
        out, crossings, _none = self._eval(sdf, False)
        self.terms, self.num_crossings = out[1:], crossings
        return out[0]
