"""The a-trous denoiser (psdr_hip_denoise_apply / _apply_adj) against the same operator written with torch ops only - what a user could do before it existed.

  python tools/denoise_timing.py [--sizes 512 2048] [--levels 5] [--guides 8] [--channels 3] [--reps 30] [--warmup 5] [--per-level] [--out FILE.json]

Workload: a square frame, seeded random guides (a ramp, a step and noise per channel, so that the weights span their range) and a seeded random image.  The torch
form states include/psdr_hip.h's operator with shifted views: per level and tap one difference of the guide frames, exp, a multiply-add into the output, then the
division by the normaliser (the transpose divides the source instead); like the HIP form it takes 1 / N_l as given, computed beforehand.  The two alternate inside one
process after the warm-ups; a call is timed with a host clock around the call and a device synchronise; apply and transpose are timed separately.  Beside the medians:
the compulsory traffic of a level - every pixel's G guide values, C image values and 1 / N read once, C values written - at the 6.29 TB/s a device-to-device copy
reaches on an MI355X, times the number of levels.

--per-level times the HIP apply and transpose for L = 1 .. levels and prints the differences: the time of each level on its own (DESIGN.md section 7d's table)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import psdr_jit_amd as psdr
from psdr_jit_amd import cabi

COPY_TBS = 6.29
H5 = [1.0 / 16, 4.0 / 16, 6.0 / 16, 4.0 / 16, 1.0 / 16]


def _views(W, H, s, i, j):
    dx, dy = s * i, s * j
    if abs(dx) >= W or abs(dy) >= H:
        return None
    return ((slice(max(0, -dy), H - max(0, dy)), slice(max(0, -dx), W - max(0, dx))),
            (slice(max(0, dy), H - max(0, -dy)), slice(max(0, dx), W - max(0, -dx))))


class TorchDenoiser:
    """the same operator, torch ops only"""

    def __init__(self, guides, W, H, L):
        self.W, self.H, self.L = W, H, L
        self.g = guides.reshape(H, W, -1)
        self.inv_n = [1.0 / self._level(None, l, norm=True) for l in range(L)]

    def _level(self, x, l, norm=False, adjoint=False):
        W, H, s = self.W, self.H, 1 << l
        g = self.g
        if norm:
            out = torch.zeros((H, W, 1), device=g.device)
        else:
            src = x * self.inv_n[l] if adjoint else x
            out = torch.zeros_like(x)
        for j in range(-2, 3):
            for i in range(-2, 3):
                v = _views(W, H, s, i, j)
                if v is None:
                    continue
                p, q = v
                hh = H5[i + 2] * H5[j + 2]
                if i == 0 and j == 0:
                    w = hh
                else:
                    d = g[p] - g[q]
                    d2 = (d * d).sum(dim=-1, keepdim=True)
                    w = torch.where(torch.isfinite(d2), torch.exp(-d2), torch.zeros_like(d2)) * hh
                out[p] += w if norm else w * src[q]
        if norm or adjoint:
            return out
        return out * self.inv_n[l]

    def apply(self, x):
        f = x.reshape(self.H, self.W, -1)
        for l in range(self.L):
            f = self._level(f, l)
        return f.reshape(self.W * self.H, -1)

    def transpose(self, y):
        f = y.reshape(self.H, self.W, -1)
        for l in range(self.L - 1, -1, -1):
            f = self._level(f, l, adjoint=True)
        return f.reshape(self.W * self.H, -1)


class RawDenoiser:
    """the four entry points called with device pointers: no autograd node, no copy"""

    def __init__(self, lib, guides, W, H, L):
        self.lib, self.h = lib, C.c_void_p()
        self.keep = guides
        rc = lib.psdr_hip_denoise_create(guides.data_ptr() if guides.shape[1] else None, int(guides.shape[1]), W, H, L, C.byref(self.h), psdr._stream_ptr())
        if rc:
            raise RuntimeError("psdr_hip_denoise_create failed")

    def _call(self, fn, x):
        out = torch.empty_like(x)
        if fn(self.h, x.data_ptr(), int(x.shape[1]), out.data_ptr(), psdr._stream_ptr()):
            raise RuntimeError("the call failed")
        return out

    def apply(self, x):
        return self._call(self.lib.psdr_hip_denoise_apply, x)

    def transpose(self, y):
        return self._call(self.lib.psdr_hip_denoise_apply_adj, y)

    def close(self):
        self.lib.psdr_hip_denoise_destroy(self.h)


def workload(size, G, Cn):
    rng = np.random.default_rng(size)
    yy, xx = np.meshgrid(np.arange(size, dtype=np.float32), np.arange(size, dtype=np.float32), indexing="ij")
    g = np.empty((size, size, G), dtype=np.float32)
    for k in range(G):
        g[..., k] = (0.01 + 0.002 * k) * (xx if k % 2 == 0 else yy) + 3.0 * ((xx + 2 * yy) > (0.7 + 0.1 * k) * size) + 0.2 * rng.standard_normal((size, size))
    x = rng.standard_normal((size * size, Cn)).astype(np.float32)
    return torch.from_numpy(g.reshape(size * size, G)).cuda(), torch.from_numpy(x).cuda()


def median_ms(fns, reps, warmup):
    """fns: name -> callable; they alternate.  -> name -> (median, min, max) in ms"""
    t = {k: [] for k in fns}
    for it in range(warmup + reps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if it >= warmup:
                t[k].append(1e3 * (time.perf_counter() - t0))
    return {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 2048])
    ap.add_argument("--levels", type=int, default=5)
    ap.add_argument("--guides", type=int, default=8)
    ap.add_argument("--channels", type=int, default=3)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--per-level", action="store_true")
    ap.add_argument("--out", default="")
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("denoise_timing.py measures on the GPU: none visible")
    lib = cabi.lib()
    res = {"levels": opt.levels, "guides": opt.guides, "channels": opt.channels, "reps": opt.reps, "sizes": {}}
    for size in opt.sizes:
        g, x = workload(size, opt.guides, opt.channels)
        n = size * size
        level_bytes = n * (4 * (opt.guides + opt.channels + 1) + 4 * opt.channels)
        floor_ms = 1e3 * opt.levels * level_bytes / (COPY_TBS * 1e12)
        entry = {"compulsory_bytes_per_level": level_bytes, "floor_ms_at_copy_rate": floor_ms}
        if opt.per_level:
            cum = []
            for L in range(1, opt.levels + 1):
                den = RawDenoiser(lib, g, size, size, L)
                m = median_ms({"apply": lambda: den.apply(x), "transpose": lambda: den.transpose(x)}, opt.reps, opt.warmup)
                den.close()
                cum.append((m["apply"][0], m["transpose"][0]))
            entry["cumulative_ms"] = cum
            prev = (0.0, 0.0)
            for l, c in enumerate(cum):
                print("%4d^2  level %d (stride %3d): apply %8.4f ms  transpose %8.4f ms   (L = %d in all: %8.4f, %8.4f; a level's compulsory bytes at the copy rate: %.4f ms)" %
                      (size, l, 1 << l, c[0] - prev[0], c[1] - prev[1], l + 1, c[0], c[1], floor_ms / opt.levels), flush=True)
                prev = c
        else:
            den = RawDenoiser(lib, g, size, size, opt.levels)
            ref = TorchDenoiser(g, size, size, opt.levels)
            a, b = den.apply(x), ref.apply(x)
            ta, tb = den.transpose(x), ref.transpose(x)
            entry["max_abs_difference"] = {"apply": float((a - b).abs().max()), "transpose": float((ta - tb).abs().max())}
            m = median_ms({"hip_apply": lambda: den.apply(x), "torch_apply": lambda: ref.apply(x),
                           "hip_transpose": lambda: den.transpose(x), "torch_transpose": lambda: ref.transpose(x)}, opt.reps, opt.warmup)
            den.close()
            entry["ms"] = {k: {"median": v[0], "min": v[1], "max": v[2]} for k, v in m.items()}
            for what in ("apply", "transpose"):
                h, t = m["hip_" + what], m["torch_" + what]
                print("%4d^2  %-9s  HIP %8.3f ms [%8.3f, %8.3f]   torch ops %9.3f ms [%9.3f, %9.3f]   torch / HIP %6.1f   compulsory bytes at %.2f TB/s: %.3f ms (HIP / that: %.1f)   largest difference %.2e" %
                      (size, what, h[0], h[1], h[2], t[0], t[1], t[2], t[0] / h[0], COPY_TBS, floor_ms, h[0] / floor_ms, entry["max_abs_difference"][what]), flush=True)
        res["sizes"][str(size)] = entry
    print(json.dumps(res))
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
