"""Adaptive sampling: spend a sample budget where the variance is (kernels: csrc/hip/adaptive.hip).

render_c_sq gives every pixel its noise estimate, and batch_pix takes a list of pixel ids with duplicates, one row and one sampler stream per entry.
This module is the piece in between:

    w = psdr.adaptive_weights(img, sq, spp)                  # per-sample standard deviation of every pixel (Neyman allocation)
    plan = psdr.PixelPlan.from_weights(w, budget)            # counts that add up to `budget` exactly, and the sorted pixel list plan.pix
    rows, rows_sq = psdr.render_c_sq(integ, sc, 0, seed=s, batch_pix=plan.pix)
    img = plan.merge(rows, spp, base=pilot, base_n=spp)      # the list's rows folded back into a frame (differentiable)

or all of it in one call, psdr.render_c_adaptive.  The differentiable case is the same recipe around renderD:

    rows = integ.renderD(sc, 0, seed=s, batch_pix=plan.pix, batch_edges=True)
    img = plan.merge(rows, sc.opts.spp)
    loss(img).backward()

Row k of a batch_edges render already carries the full-frame edge derivative of its pixel, so the mean over a pixel's rows leaves the edge terms
as they are and averages only the interior term over more samples.

Everything here runs on torch's current stream without a device-to-host copy: the host knows the length of the list (the budget) beforehand.
One GPU only: under an initialised torch.distributed group of more than one rank the calls raise."""
import torch as _torch

from . import cabi as _cabi

MAIN_SEED_OFFSET = 1 << 24          # render_c_adaptive: the list's seed is the pilot's plus this.  A stream is (seed + pixel, lane) and a frame has at most 2^24
#                                     pixels here, so no entry of the list repeats a stream of the pilot


def _single_gpu(what):
    from . import _shard
    if _shard()[1] > 1:
        raise RuntimeError("%s: adaptive sampling runs on one GPU, torch.distributed is initialised with %d ranks" % (what, _shard()[1]))


def _f32(t, dev):
    return t.detach().to(dev, _torch.float32).contiguous()


def adaptive_weights(mean, sq, n, mode="absolute", eps=1e-3):
    """The weight map of the Neyman allocation from a render and its sample squares: float32 [n_pixels].

        absolute:  w_p = sqrt(sum_c max(n * variance_from_sq(mean, sq, n)[p, c], 0))          the per-sample standard deviation, channels added in variance
        relative:  w_p = that / (sum_c mean[p, c] + eps)                                       the same relative to the pixel's brightness

    n * variance_from_sq is the variance of ONE sample of the pixel (variance_from_sq is that of the mean of n).  Among all ways to split a budget
    N = sum n_p, the sum over the pixels of sigma_p^2 / n_p is smallest for n_p proportional to sigma_p: that is "absolute".  "relative" minimises the
    summed squared RELATIVE error instead, which is what a tone-mapped image shows; eps (in units of radiance) keeps black pixels finite.
    mean, sq: [n_pixels, channels] tensors as render_c_sq / render_d_fwd_sq return them; n = samples_behind(scene, term) > 1."""
    from . import variance_from_sq
    if mode not in ("absolute", "relative"):
        raise ValueError("adaptive_weights: mode is 'absolute' or 'relative', got %r" % (mode,))
    sigma = (variance_from_sq(mean, sq, n) * n).clamp_min(0.0).sum(dim=-1).sqrt()
    if mode == "relative":
        sigma = sigma / (mean.sum(dim=-1) + eps)
    return sigma


class _MergeFn(_torch.autograd.Function):
    """plan.merge; the backward is psdr_hip_adaptive_merge_adj"""

    @staticmethod
    def forward(ctx, plan, rows, rows_n, base, base_n):
        ctx.plan, ctx.rows_n, ctx.base_n = plan, rows_n, base_n
        ctx.rows_like = (rows.device, rows.dtype)
        ctx.base_like = (base.device, base.dtype) if base is not None else None
        ctx.channels = int(rows.shape[1])
        return plan._fold(rows, rows_n, base, base_n, 0)

    @staticmethod
    def backward(ctx, g):
        from . import _stream_ptr
        plan, ch = ctx.plan, ctx.channels
        g = _f32(g, plan.counts.device)
        d_rows = _torch.empty((plan.total, ch), dtype=_torch.float32, device=g.device)
        d_base = _torch.empty((plan.n, ch), dtype=_torch.float32, device=g.device) if ctx.base_like is not None and ctx.needs_input_grad[3] else None
        _cabi.check(_cabi.lib().psdr_hip_adaptive_merge_adj(plan.offsets.data_ptr(), plan.n, plan.total, ch, g.data_ptr(), ctx.rows_n, ctx.base_n,
                                                            d_rows.data_ptr() if plan.total else None, d_base.data_ptr() if d_base is not None else None, _stream_ptr()))
        return None, d_rows.to(*ctx.rows_like), None, (d_base.to(*ctx.base_like) if d_base is not None else None), None


class PixelPlan:
    """A sample allocation over the n pixels of a frame and the pixel list that realises it.

        counts  [n] int32      entries of pixel p;  counts.sum() == total, exactly
        offsets [n + 1] int32  exclusive scan of counts;  offsets[n] == total
        pix     [total] int32  the list, sorted by pixel: pixel p occupies entries offsets[p] .. offsets[p + 1] - 1 (neighbouring lanes of the path kernels stay on
                               neighbouring pixels).  total == 0: an empty tensor, which the batch entry points refuse - do not render it
    all on the render device.  `seed` is set by render_c_adaptive: the seed of the render over `pix`."""

    def __init__(self, counts, offsets, pix, n, total):
        self.counts, self.offsets, self.pix, self.n, self.total = counts, offsets, pix, int(n), int(total)
        self.seed = None

    @classmethod
    def from_weights(cls, weights, budget, min_count=0):
        """The allocation of `budget` list entries in proportion to `weights` (any shape, one value per pixel in pixel order; NaN, Inf and values <= 0 count as 0;
        a map without any positive value gives the uniform allocation), at least `min_count` per pixel.  Cumulative rounding of the quantised weights: the counts add
        up to `budget` exactly and each is within one of min_count + (budget - n min_count) q_p / sum q (psdr_hip_adaptive_counts, include/psdr_hip.h).  No
        synchronisation: three small launches for the counts and one for the list.  budget <= 2^31 - 1, n <= 2^24; budget == 0 gives an empty plan."""
        from . import _device, _stream_ptr
        _single_gpu("PixelPlan.from_weights")
        dev = _device()
        w = _f32(_torch.as_tensor(weights), dev).reshape(-1)
        n, budget, min_count = int(w.numel()), int(budget), int(min_count)
        L = _cabi.lib()
        counts = _torch.empty(n, dtype=_torch.int32, device=dev)
        offsets = _torch.empty(n + 1, dtype=_torch.int32, device=dev)
        scratch = _torch.empty(int(L.psdr_hip_adaptive_scratch_bytes()), dtype=_torch.uint8, device=dev)
        _cabi.check(L.psdr_hip_adaptive_counts(w.data_ptr() if n else None, n, budget, min_count, counts.data_ptr() if n else None, offsets.data_ptr(), scratch.data_ptr(), _stream_ptr()))
        pix = _torch.empty(budget, dtype=_torch.int32, device=dev)
        _cabi.check(L.psdr_hip_adaptive_expand(offsets.data_ptr(), n, budget, pix.data_ptr() if budget else None, _stream_ptr()))
        return cls(counts, offsets, pix, n, budget)

    def _fold(self, rows, rows_n, base, base_n, square):
        from . import _stream_ptr
        _single_gpu("PixelPlan.merge")
        dev = self.counts.device
        if rows.dim() != 2 or int(rows.shape[0]) != self.total:
            raise ValueError("PixelPlan: expected rows of shape [%d, channels], got %s" % (self.total, tuple(rows.shape)))
        ch = int(rows.shape[1])
        if base is None:
            if base_n != 0:
                raise ValueError("PixelPlan: base_n = %r without a base" % (base_n,))
        elif tuple(base.shape) != (self.n, ch):
            raise ValueError("PixelPlan: expected a base of shape [%d, %d], got %s" % (self.n, ch, tuple(base.shape)))
        r = _f32(rows, dev)
        b = _f32(base, dev) if base is not None else None
        out = _torch.empty((self.n, ch), dtype=_torch.float32, device=dev)
        _cabi.check(_cabi.lib().psdr_hip_adaptive_merge(self.offsets.data_ptr(), self.n, self.total, ch, r.data_ptr() if self.total else None, float(rows_n),
                                                        b.data_ptr() if b is not None else None, float(base_n), int(square), out.data_ptr(), _stream_ptr()))
        return out

    def merge(self, rows, rows_n, base=None, base_n=0):
        """The rows of a render over `pix` folded into a frame [n, channels]:

            out[p] = (base_n base[p] + rows_n sum_k rows[k]) / (base_n + rows_n counts[p])          k over the entries of pixel p

        rows_n: the samples every row averages (opts.spp of the render); base: an earlier frame that averaged base_n samples per pixel (the pilot), or None.  A pixel
        without entries and without base is 0.  Differentiable in rows and base (the backward is a gather, psdr_hip_adaptive_merge_adj); the order of every sum
        is fixed, so two calls give the same bits."""
        return _MergeFn.apply(self, rows, float(rows_n), base, float(base_n))

    def merge_sq(self, rows_sq, rows_n, base_sq=None, base_n=0):
        """The sum of squared sample contributions of the frame `merge` returns, from those of its parts (render_c_sq's second result): a sample of a row adds
        x / rows_n to the row and x / n_tot to the merged pixel, so a row's squares weigh (rows_n / n_tot)^2 and the base's (base_n / n_tot)^2, n_tot = samples(...).
        Detached, like every buffer of squares."""
        return self._fold(rows_sq, float(rows_n), base_sq, float(base_n), 1)

    def samples(self, rows_n, base_n=0):
        """n_tot, the samples behind every pixel of the merged frame: float32 [n] = base_n + rows_n counts"""
        return self.counts.to(_torch.float32) * float(rows_n) + float(base_n)

    def variance(self, img, sq, rows_n, base_n=0):
        """variance_from_sq's formula with the per-pixel n of samples(...): (sq - img^2 / n) n / (n - 1), and 0 where n <= 1 (no variance from one sample)"""
        n = self.samples(rows_n, base_n).to(device=img.device, dtype=img.dtype)[:, None]          # (the counts are exact in float32; the formula runs in img's precision)
        ok = n > 1
        n1 = _torch.where(ok, n, _torch.full_like(n, 2.0))
        return _torch.where(ok, (sq - img * img / n1) * (n1 / (n1 - 1)), _torch.zeros_like(sq))


def render_c_adaptive(integrator, scene, budget, sensor_id=0, seed=-1, pilot_spp=None, mode="absolute", min_count=0, reuse_pilot=True):
    """renderC with its samples placed by a pilot's noise estimate: returns (img, sq, plan), img and sq float32 [n_pixels, 3] and detached.

      1. a pilot render_c_sq of the whole frame at pilot_spp samples per pixel (default: the scene's spp; it needs at least 2 for a variance), seed `seed`
      2. plan = PixelPlan.from_weights(adaptive_weights(pilot, pilot_sq, pilot_spp, mode), budget / spp, min_count)
      3. one render_c_sq over plan.pix at the scene's spp, seed plan.seed = seed + MAIN_SEED_OFFSET (no stream of the pilot is drawn again)
      4. img = plan.merge(rows, spp, pilot, pilot_spp), sq = plan.merge_sq(...); plan.variance(img, sq, spp, pilot_spp) is the variance of img

    budget: the SAMPLES of step 3, a multiple of the scene's spp (an entry of the list is one row of spp samples: set spp = 1 for the finest allocation).
    The frame then rests on n_pixels * pilot_spp + budget samples, plan.samples(spp, pilot_spp) per pixel.  budget == 0 returns the pilot and launches no second render.

    reuse_pilot=True mixes the pilot into the result.  That is the usual estimator and it is slightly biased: the pilot's samples also chose the counts, so a pixel
    whose pilot came out dark AND quiet keeps few samples and stays dark.  reuse_pilot=False returns the list's rows alone, which are independent of the
    counts - unbiased, at the price of the pilot's samples (give min_count >= 1, or a pixel without entries is 0).  seed: required, as for every pixel list.
    opts.spp is changed for the pilot when pilot_spp differs and is restored on every way out."""
    from . import render_c_sq
    _single_gpu("render_c_adaptive")
    if seed == -1:
        raise ValueError("render_c_adaptive: seed must be set (a pixel list is rendered)")
    opts = scene.opts
    spp = int(opts.spp)
    pilot_spp = spp if pilot_spp is None else int(pilot_spp)
    budget = int(budget)
    if pilot_spp < 2:
        raise ValueError("render_c_adaptive: the pilot needs at least 2 samples per pixel for a variance, got %d" % pilot_spp)
    if spp < 1 or budget < 0 or budget % spp:
        raise ValueError("render_c_adaptive: budget = %d must be a non-negative multiple of the scene's spp = %d" % (budget, spp))
    if budget == 0 and not reuse_pilot:
        raise ValueError("render_c_adaptive: budget = 0 with reuse_pilot=False leaves no sample")

    def set_spp(value):
        if int(opts.spp) != value:
            opts.spp = value
            scene.configure(scene.__dict__.get("_psdr_active", []))          # the device copy of the options follows

    try:
        set_spp(pilot_spp)
        pilot, pilot_sq = render_c_sq(integrator, scene, sensor_id, seed=seed)
    finally:
        set_spp(spp)
    plan = PixelPlan.from_weights(adaptive_weights(pilot, pilot_sq, pilot_spp, mode), budget // spp, min_count)
    plan.seed = (int(seed) + MAIN_SEED_OFFSET) & 0x7fffffff
    if plan.total == 0:
        return pilot, pilot_sq, plan
    rows, rows_sq = render_c_sq(integrator, scene, sensor_id, seed=plan.seed, batch_pix=plan.pix)
    if not reuse_pilot:
        return plan.merge(rows, spp), plan.merge_sq(rows_sq, spp), plan
    return plan.merge(rows, spp, pilot, pilot_spp), plan.merge_sq(rows_sq, spp, pilot_sq, pilot_spp), plan
