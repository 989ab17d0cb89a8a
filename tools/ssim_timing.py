"""The SSIM loss, value plus gradient (psdr_hip_ssim_eval through psdr.SSIMLoss), against the same loss written with torch ops only - what a user could do before it
existed.  A yardstick, not a comparison against this code.

  python tools/ssim_timing.py [--reps 30] [--warmup 5] [--out FILE.json] [--only-fused SIDE]

Workloads: 512 x 512 and 2048 x 2048, C = 3, K = 11, sigma = 1.5, padding "same", no mask.  Candidates, alternating inside one process after the warm-up:
  fused       ss.value_and_grad(img, target)                                  three launches
  autograd    ss(img, target).backward() with img a leaf                     the same three launches behind torch's autograd engine
  torch       the loss on the [W H, C] layout with torch ops: reshape and permute, five F.conv2d(groups=3, padding=5) with the outer-product window, the pointwise
              formula, the mean; .backward() with img a leaf
Two clocks per candidate: `call` is a host clock around one call that ends in a device synchronise (median of --reps calls, min - max), what a step that reads the
loss every iteration pays; `queued` is device events around --reps calls queued back to back, divided by --reps: what the stream is busy for when nothing waits.
The table also gives whether ten gradients of the same input agree bit for bit, the relative l2 distance between the two forms' gradients, and the floors at the
6.29 TB/s device-copy rate DESIGN.md uses: `must` is one read of both images and one write of the gradient (3 frames), `moves` is what the three kernels move through
their ports without counting the halo's second reads (k_stat reads 2 and writes 4, k_grad reads 3 + 2 and writes 1: 12 frames).
--only-fused SIDE runs nothing but 40 fused calls at SIDE x SIDE: the process for a kernel trace of its own."""
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
C, K, SIGMA = 3, 11, 1.5


def torch_form(img, target, W, H, win, c1, c2):
    """the definition with torch ops; img [W H, C] -> 0-d loss"""
    x = img.reshape(H, W, C).permute(2, 0, 1)[None]
    y = target.reshape(H, W, C).permute(2, 0, 1)[None]
    conv = lambda t: F.conv2d(t, win, padding=K // 2, groups=C)
    mu_x, mu_y = conv(x), conv(y)
    s_xx, s_yy, s_xy = conv(x * x) - mu_x * mu_x, conv(y * y) - mu_y * mu_y, conv(x * y) - mu_x * mu_y
    S = ((2 * mu_x * mu_y + c1) * (2 * s_xy + c2)) / ((mu_x * mu_x + mu_y * mu_y + c1) * (s_xx + s_yy + c2))
    return 1 - S.mean()


def floors(W, H):
    frame = 4 * C * W * H
    must, moves = 3 * frame, 12 * frame
    return {"must_bytes": must, "moves_bytes": moves, "must_ms": 1e3 * must / COPY_BYTES_PER_S, "moves_ms": 1e3 * moves / COPY_BYTES_PER_S}


def inputs(W, H):
    rng = np.random.default_rng(1)
    img = torch.from_numpy(rng.random((W * H, C), dtype=np.float32)).cuda()
    target = (0.75 * img + 0.25 * torch.from_numpy(rng.random((W * H, C), dtype=np.float32)).cuda()).contiguous()
    return img, target


def measure(W, H, reps, warmup):
    ss = psdr.SSIMLoss(W, H, channels=C, window=K, sigma=SIGMA)
    img, target = inputs(W, H)
    leaf = img.clone().requires_grad_()
    g = torch.from_numpy(psdr.gaussian_window(K, SIGMA)).cuda()
    win = torch.outer(g, g)[None, None].repeat(C, 1, 1, 1).contiguous()

    def fused():
        return ss.value_and_grad(img, target)

    def autograd():
        leaf.grad = None
        loss = ss(leaf, target)
        loss.backward()
        return loss.detach(), leaf.grad

    def torch_ops():
        leaf.grad = None
        loss = torch_form(leaf, target, W, H, win, ss.c1, ss.c2)
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
    res = {"W": W, "H": H, "C": C, "K": K, "sigma": SIGMA, "reps": reps, "warmup": warmup, "floor": floors(W, H), "bit_stable_over_10_runs": stable,
           "loss": {key: float(last[key][0]) for key, _ in cands},
           "rel_l2_gradient_vs_torch": float((last["fused"][1].double() - last["torch"][1].double()).norm() / last["torch"][1].double().norm()),
           "autograd_equals_fused": bool(torch.equal(last["fused"][1], last["autograd"][1]) and torch.equal(last["fused"][0], last["autograd"][0]))}
    print("%d x %d, C = %d, K = %d" % (W, H, C, K))
    for key, _ in cands:
        a = np.asarray(t[key])
        res[key] = {"call_median_ms": float(np.median(a)), "call_min_ms": float(a.min()), "call_max_ms": float(a.max()), "queued_ms": queued[key]}
        print("  %-9s call %8.4f ms [%8.4f, %8.4f]   queued %8.4f ms   bit-stable over 10 runs: %s" % (key, np.median(a), a.min(), a.max(), queued[key], stable[key]))
    f = res["floor"]
    print("  floor: must %.4f ms (%d bytes), moves %.4f ms (%d bytes); loss fused %.9g torch %.9g; gradient rel l2 against torch %.2e; autograd == fused: %s" %
          (f["must_ms"], f["must_bytes"], f["moves_ms"], f["moves_bytes"], res["loss"]["fused"], res["loss"]["torch"], res["rel_l2_gradient_vs_torch"], res["autograd_equals_fused"]),
          flush=True)
    return res


def only_fused(side):
    ss = psdr.SSIMLoss(side, side, channels=C, window=K, sigma=SIGMA)
    img, target = inputs(side, side)
    for _ in range(40):
        ss.value_and_grad(img, target)
    torch.cuda.synchronize()
    print("40 fused calls at %d x %d, loss %.9g" % (side, side, float(ss.value_and_grad(img, target)[0])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--only-fused", type=int, default=0)
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ssim_timing.py measures on the GPU: none visible")
    if opt.only_fused:
        return only_fused(opt.only_fused)
    res = [measure(side, side, opt.reps, opt.warmup) for side in (512, 2048)]
    print(json.dumps(res))
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
