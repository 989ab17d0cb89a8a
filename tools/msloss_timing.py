"""The multi-scale loss, value plus gradient (psdr_hip_msloss_eval through psdr.MultiScaleLoss), against the same loss written with torch ops only - what a user
could do before it existed.  A yardstick, not a comparison against this code.

  python tools/msloss_timing.py [--reps 30] [--warmup 5] [--out FILE.json]

Workloads: 512 x 512 and 2048 x 2048, C = 3, every level down to 1 x 1 (10 and 12 levels), norm l1 and l2, no weight.  Candidates, alternating inside one process
after the warm-up:
  fused       ms.value_and_grad(img, target)                                  three launches
  autograd    ms(img, target).backward() with img a leaf                     the same three launches behind torch's autograd engine
  torch       the loss on the [W H, C] layout with torch ops: reshape and permute, then per level rho, mean and
              F.avg_pool2d(x, 2, ceil_mode=True, count_include_pad=False); .backward() with img a leaf
Two clocks per candidate: `call` is a host clock around one call that ends in a device synchronise (median of --reps calls, min - max), what a step that reads
the loss every iteration pays; `queued` is device events around --reps calls queued back to back, divided by --reps: what the stream is busy for when nothing waits.
The table also gives whether ten gradients of the same input agree bit for bit (the fused ones do by construction; both are checked), the difference between the
two forms, and the floors at the 6.29 TB/s device-copy rate DESIGN.md uses: `must` is one read of both images and one write of the gradient (3 frames), `moves` is
what the three kernels move (both images read, the pyramid written and read back, the gradient written: 17/3 frames)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import torch.nn.functional as F

import psdr_jit_amd as psdr

COPY_BYTES_PER_S = 6.29e12
C = 3


def torch_form(img, target, W, H, norm, levels):
    """the definition with torch ops; img [W H, C] -> 0-d loss"""
    x = (img - target).reshape(H, W, C).permute(2, 0, 1)[None]
    loss = None
    for l in range(levels):
        ll = x.abs().mean() if norm == "l1" else x.square().mean()
        loss = ll if loss is None else loss + ll
        if l + 1 < levels:
            x = F.avg_pool2d(x, 2, ceil_mode=True, count_include_pad=False)
    return loss


def floors(W, H, levels):
    frame = 4 * C * W * H
    pyr = 4 * C * sum(w * h for w, h in psdr.pyramid_shapes(W, H, levels))
    must, moves = 3 * frame, 3 * frame + 2 * pyr
    return {"must_bytes": must, "moves_bytes": moves, "must_ms": 1e3 * must / COPY_BYTES_PER_S, "moves_ms": 1e3 * moves / COPY_BYTES_PER_S}


def measure(W, H, norm, reps, warmup):
    ms = psdr.MultiScaleLoss(W, H, channels=C, norm=norm)
    rng = np.random.default_rng(1)
    img = torch.from_numpy(rng.standard_normal((W * H, C)).astype(np.float32)).cuda()
    target = torch.from_numpy(rng.standard_normal((W * H, C)).astype(np.float32)).cuda()
    leaf = img.clone().requires_grad_()

    def fused():
        return ms.value_and_grad(img, target)

    def autograd():
        leaf.grad = None
        loss = ms(leaf, target)
        loss.backward()
        return loss.detach(), leaf.grad

    def torch_ops():
        leaf.grad = None
        loss = torch_form(leaf, target, W, H, norm, ms.levels)
        loss.backward()
        return loss.detach(), leaf.grad

    cands = [("fused", fused), ("autograd", autograd), ("torch", torch_ops)]
    t, last = {k: [] for k, _ in cands}, {}
    for k in range(warmup + reps):
        for key, fn in cands:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            if k >= warmup:
                t[key].append(1e3 * (time.perf_counter() - t0))
            last[key] = (out[0].clone(), out[1].clone())
    queued = {}
    for key, fn in cands:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        queued[key] = e0.elapsed_time(e1) / reps
    stable = {key: all(torch.equal(fn()[1], last[key][1]) for _ in range(10)) for key, fn in cands}
    res = {"W": W, "H": H, "C": C, "levels": ms.levels, "norm": norm, "reps": reps, "warmup": warmup, "floor": floors(W, H, ms.levels), "bit_stable_over_10_runs": stable,
           "loss": {key: float(last[key][0]) for key, _ in cands},
           "rel_l2_gradient_vs_torch": float((last["fused"][1].double() - last["torch"][1].double()).norm() / last["torch"][1].double().norm()),
           "autograd_equals_fused": bool(torch.equal(last["fused"][1], last["autograd"][1]) and torch.equal(last["fused"][0], last["autograd"][0]))}
    print("%d x %d, C = %d, %d levels, %s" % (W, H, C, ms.levels, norm))
    for key, _ in cands:
        a = np.asarray(t[key])
        res[key] = {"call_median_ms": float(np.median(a)), "call_min_ms": float(a.min()), "call_max_ms": float(a.max()), "queued_ms": queued[key]}
        print("  %-9s call %8.4f ms [%8.4f, %8.4f]   queued %8.4f ms   bit-stable over 10 runs: %s" % (key, np.median(a), a.min(), a.max(), queued[key], stable[key]))
    f = res["floor"]
    print("  floor: must %.4f ms (%d bytes), moves %.4f ms (%d bytes); loss fused %.9g torch %.9g; gradient rel l2 against torch %.2e; autograd == fused: %s" %
          (f["must_ms"], f["must_bytes"], f["moves_ms"], f["moves_bytes"], res["loss"]["fused"], res["loss"]["torch"], res["rel_l2_gradient_vs_torch"], res["autograd_equals_fused"]),
          flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("msloss_timing.py measures on the GPU: none visible")
    res = [measure(side, side, norm, opt.reps, opt.warmup) for side in (512, 2048) for norm in ("l1", "l2")]
    print(json.dumps(res))
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
