"""What adaptive sampling costs and what it buys, on the README box (512 x 512, 32 samples, depth 3) and on BASELINE config 5's scene (512 x 512,
16 samples, the 82 k-triangle mesh under the environment map).

Cost.  One adaptive frame is: render_c_sq of the full frame (the pilot), weights + PixelPlan.from_weights (three scan launches and the list), render_c_sq over the list,
plan.merge + plan.merge_sq, and - in an optimisation - the backward of plan.merge.  The list has one entry per pixel on average (budget = W H spp samples), so the two
renders cost about the same.  The five pieces alternate, ROUNDS windows of REPS calls each; printed per piece: the median window and the spread (min - max) of its
windows, and the share of plan + fold + transpose in the two renders they sit between.

Benefit.  The mean squared error of render_c_adaptive (pilot of spp / 2 samples, the other half of the samples placed by it in entries of spp / 8) against a uniform
renderC with the same number of samples, both against one reference of REF_FRAMES frames; SEEDS seeds each, printed as mean and standard deviation across the seeds.
python tools/adaptive_timing.py [--small]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import __graft_entry__; __graft_entry__.build()
import psdr_jit_amd as psdr
import scenes, product

small = "--small" in sys.argv          # a rehearsal of the script, not a measurement
ROUNDS = 5
SEEDS = 4 if small else 16
REF_FRAMES = 4 if small else 64


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def set_spp(sc, spp):
    if sc.opts.spp != spp:
        sc.opts.spp = spp
        sc.configure(sc.__dict__.get("_psdr_active", []))


def cost(name, sc, integ, spp, reps, mode):
    n = sc.opts.width * sc.opts.height
    set_spp(sc, spp)
    pilot, pilot_sq = psdr.render_c_sq(integ, sc, 0, seed=1)
    state = {}

    def plan():
        state["plan"] = psdr.PixelPlan.from_weights(psdr.adaptive_weights(pilot, pilot_sq, spp, mode), n)
    plan()
    p = state["plan"]
    rows, rows_sq = psdr.render_c_sq(integ, sc, 0, seed=2, batch_pix=p.pix)
    g = torch.ones((n, 3), device="cuda")
    leaf = rows.clone().requires_grad_()
    merged = p.merge(leaf, spp, pilot, spp)
    pieces = [("render, full frame", lambda: psdr.render_c_sq(integ, sc, 0, seed=1)),
              ("weights + plan + list", plan),
              ("render, the list", lambda: psdr.render_c_sq(integ, sc, 0, seed=2, batch_pix=p.pix)),
              ("merge + merge_sq", lambda: (p.merge(rows, spp, pilot, spp), p.merge_sq(rows_sq, spp, pilot_sq, spp))),
              ("transpose of merge", lambda: merged.backward(g, retain_graph=True))]
    for _ in range(2):
        for _label, fn in pieces:
            fn()
    torch.cuda.synchronize()
    t = np.array([[window(fn, reps) for _label, fn in pieces] for _ in range(ROUNDS)])
    med = np.median(t, axis=0)
    for k, (label, _fn) in enumerate(pieces):
        print("%-12s %-24s %9.4f ms (%.4f - %.4f)" % (name, label, med[k], t[:, k].min(), t[:, k].max()))
    share = (t[:, 1] + t[:, 3] + t[:, 4]) / (t[:, 0] + t[:, 2])
    counts = p.counts.cpu().numpy()
    print("%-12s plan + fold + transpose over the two renders: %.4f %% (%.4f - %.4f); list of %d entries, counts %d - %d, %.1f %% of the pixels without entries" %
          (name, 100 * np.median(share), 100 * share.min(), 100 * share.max(), p.total, counts.min(), counts.max(), 100.0 * (counts == 0).mean()))


def benefit(name, sc, integ, spp, mode):
    n = sc.opts.width * sc.opts.height
    set_spp(sc, spp)
    ref = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    for k in range(REF_FRAMES):
        ref += integ.renderC(sc, 0, seed=900001 + 7919 * k).double()
    ref /= REF_FRAMES
    uniform = [float(((integ.renderC(sc, 0, seed=101 + 31 * k).double() - ref) ** 2).mean()) for k in range(SEEDS)]
    entry = max(1, spp // 8)
    set_spp(sc, entry)
    try:
        adaptive, last = [], None
        for k in range(SEEDS):
            img, _sq, last = psdr.render_c_adaptive(integ, sc, n * spp // 2, seed=101 + 31 * k, pilot_spp=spp // 2, mode=mode)
            adaptive.append(float(((img.double() - ref) ** 2).mean()))
    finally:
        set_spp(sc, spp)
    counts = last.counts.cpu().numpy()
    u, a = np.array(uniform), np.array(adaptive)
    # the reference's own noise adds the same amount, var / (REF_FRAMES spp), to both sides
    print("%-12s MSE against %d x %d samples, %d seeds, %s weights: uniform %d spp %.4e +- %.2e   adaptive (%d pilot + %d placed, entries of %d) %.4e +- %.2e   ratio %.3f; counts %d - %d" %
          (name, REF_FRAMES, spp, SEEDS, mode, spp, u.mean(), u.std(ddof=1), spp // 2, spp // 2, entry, a.mean(), a.std(ddof=1), a.mean() / u.mean(), counts.min(), counts.max()))


res = 64 if small else 512
box = product.build_scene(scenes.cbox_scene(res, res, 32, 0, 0, param="box_x"))
cfg5 = product.build_scene(scenes.config5_scene(res, res, 16, 0, 0, level=1 if small else 6, env_res=(64, 32) if small else (1024, 512)))
integ = psdr.PathTracer(3)
cost("README box", box, integ, 32, 3 if small else 20, "absolute")
cost("config 5", cfg5, integ, 16, 2 if small else 5, "absolute")
for mode in ("absolute", "relative"):
    benefit("README box", box, integ, 32, mode)
    benefit("config 5", cfg5, integ, 16, mode)
