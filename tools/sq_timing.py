"""What the sample squares cost: psdr_hip_render_c against psdr_hip_render_c_sq and psdr_hip_render_d_fwd against psdr_hip_render_d_fwd_sq, on the README box (512 x 512,
32 / 32 / 32 samples, depth 3: scene in LDS, the plain calls run the lean kernels) and on BASELINE config 5 (512 x 512, 16 / 16 / 16, the 82 k-triangle mesh under the
environment map, secondary-edge guiding: BVH scene, decoupled kernels, forked terms).  The two calls of a pair alternate, ROUNDS windows of REPS calls each; printed per
call: the median window and the spread (min - max) of its windows, so that a difference can be read against the plain call's own repeats.   python tools/sq_timing.py [--small]"""
import os, sys, ctypes as C
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import __graft_entry__; __graft_entry__.build()
import psdr_jit_amd as psdr
from psdr_jit_amd import cabi
import scenes, product

small = "--small" in sys.argv          # a rehearsal of the script, not a measurement
ROUNDS = 5
L = cabi.lib()


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def pair(label, plain, with_sq, reps):
    for _ in range(2):
        plain(); with_sq()
    torch.cuda.synchronize()
    t = np.array([[window(plain, reps), window(with_sq, reps)] for _ in range(ROUNDS)])
    med = np.median(t, axis=0)
    print("%-28s plain %8.3f ms (%.3f - %.3f)   with squares %8.3f ms (%.3f - %.3f)   ratio %.3f" %
          (label, med[0], t[:, 0].min(), t[:, 0].max(), med[1], t[:, 1].min(), t[:, 1].max(), med[1] / med[0]))


def measure(name, spec, depth, reps, guiding=None):
    sc = product.build_scene(spec)
    n = spec.width * spec.height
    buf = torch.empty((4, n, 3), dtype=torch.float32, device="cuda")
    p = [buf[k].data_ptr() for k in range(4)]
    h = sc._hip_handle()
    g = None
    if guiding is not None:
        integ = psdr.PathTracer(depth)
        integ.preprocess_secondary_edges(sc, 0, guiding, 1, 0)
        g = integ._guiding_handle(0)
    a = cabi.make_args(max_depth=depth, seeds=(1, 2, 3), terms=7, guiding=g)          # (the C ABI's default, as bench.py: every primary-edge sample is traced)
    pair(name + " render_c", lambda: cabi.check(L.psdr_hip_render_c(h, C.byref(a), p[0], None)),
         lambda: cabi.check(L.psdr_hip_render_c_sq(h, C.byref(a), p[0], p[2], None)), reps)
    pair(name + " render_d_fwd", lambda: cabi.check(L.psdr_hip_render_d_fwd(h, C.byref(a), p[0], p[1], None)),
         lambda: cabi.check(L.psdr_hip_render_d_fwd_sq(h, C.byref(a), p[0], p[1], p[2], p[3], None)), reps)
    print("%-28s checksums %.6f %.6f %.6f %.6f" % (name, *[float(buf[k].double().sum()) for k in range(4)]))


res = 64 if small else 512
measure("README box", scenes.cbox_scene(res, res, 32, 32, 32, param="box_x"), 3, 3 if small else 20)
measure("config 5", scenes.config5_scene(res, res, 16, 16, 16, level=1 if small else 6, env_res=(64, 32) if small else (1024, 512)), 3, 2 if small else 3,
        guiding=[40, 4, 4, 8] if small else [2000, 5, 5, 32])
