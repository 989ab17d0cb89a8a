"""The variance-guided a-trous denoiser (psdr_hip_vdenoise_apply / _frozen / _frozen_adj) against the plain denoiser's apply (psdr_hip_denoise_apply), the yardstick.

  python tools/vdenoise_timing.py [--sizes 512 2048] [--levels 5] [--guides 8] [--channels 3] [--reps 30] [--warmup 5] [--out FILE.json]

Workload: a square frame, the seeded random guides and image of tools/denoise_timing.py, and a seeded variance spread over three decades.  The entry points are called
with device pointers (no autograd node, no copy); the four calls alternate inside one process after the warm-ups; a call is timed with a host clock around the call and
a device synchronise.  Beside the medians: the bytes of the record the handle owns (12 L W H)."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

import psdr_jit_amd as psdr
from psdr_jit_amd import cabi

import denoise_timing as dt


class RawVarianceDenoiser:
    """the entry points called with device pointers"""

    def __init__(self, lib, guides, W, H, L, k=0.25, eps=1e-12):
        self.lib, self.h, self.k, self.eps = lib, C.c_void_p(), k, eps
        self.keep = guides
        if lib.psdr_hip_vdenoise_create(guides.data_ptr() if guides.shape[1] else None, int(guides.shape[1]), W, H, L, C.byref(self.h), psdr._stream_ptr()):
            raise RuntimeError("psdr_hip_vdenoise_create failed")

    def apply(self, x, v):
        out, v_out = torch.empty_like(x), torch.empty_like(v)
        a = (C.c_float * 3)(0.2126, 0.7152, 0.0722) if x.shape[1] == 3 else (C.c_float * 1)(1.0)
        if self.lib.psdr_hip_vdenoise_apply(self.h, x.data_ptr(), int(x.shape[1]), v.data_ptr(), a, self.k, self.eps, out.data_ptr(), v_out.data_ptr(), psdr._stream_ptr()):
            raise RuntimeError("the call failed")
        return out

    def _call(self, fn, x):
        out = torch.empty_like(x)
        if fn(self.h, x.data_ptr(), int(x.shape[1]), out.data_ptr(), psdr._stream_ptr()):
            raise RuntimeError("the call failed")
        return out

    def frozen(self, u):
        return self._call(self.lib.psdr_hip_vdenoise_frozen, u)

    def transpose(self, y):
        return self._call(self.lib.psdr_hip_vdenoise_frozen_adj, y)

    def close(self):
        self.lib.psdr_hip_vdenoise_destroy(self.h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 2048])
    ap.add_argument("--levels", type=int, default=5)
    ap.add_argument("--guides", type=int, default=8)
    ap.add_argument("--channels", type=int, default=3, choices=(1, 3))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vdenoise_timing.py measures on the GPU: none visible")
    lib = cabi.lib()
    res = {"levels": opt.levels, "guides": opt.guides, "channels": opt.channels, "reps": opt.reps, "sizes": {}}
    for size in opt.sizes:
        g, x = dt.workload(size, opt.guides, opt.channels)
        v = torch.from_numpy((10.0 ** np.random.default_rng(size + 1).uniform(-3, 0, size * size)).astype(np.float32)).cuda()
        plain = dt.RawDenoiser(lib, g, size, size, opt.levels)
        den = RawVarianceDenoiser(lib, g, size, size, opt.levels)
        out = den.apply(x, v)
        same = bool(torch.equal(den.frozen(x), out))
        m = dt.median_ms({"denoiser_apply": lambda: plain.apply(x), "apply": lambda: den.apply(x, v), "frozen": lambda: den.frozen(x), "transpose": lambda: den.transpose(x)},
                         opt.reps, opt.warmup)
        plain.close()
        den.close()
        record = 12 * opt.levels * size * size
        entry = {"ms": {k: {"median": t[0], "min": t[1], "max": t[2]} for k, t in m.items()}, "record_bytes": record, "frozen_equals_apply": same}
        base = m["denoiser_apply"][0]
        for what in ("denoiser_apply", "apply", "frozen", "transpose"):
            t = m[what]
            print("%4d^2  %-14s  %8.3f ms [%8.3f, %8.3f]   x %5.2f of Denoiser's apply" % (size, what, t[0], t[1], t[2], t[0] / base), flush=True)
        print("%4d^2  record %.1f MB; frozen(x) equals apply(x, v) bit for bit: %s" % (size, record / 1e6, same), flush=True)
        res["sizes"][str(size)] = entry
    print(json.dumps(res))
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
