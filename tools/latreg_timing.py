"""The lattice regularisers (psdr.LatticeRegularizer: value and gradient in three launches) against the same three terms written with torch ops only, the form DMTet /
nvdiffrec-style code uses: shifted views of the lattice, binary_cross_entropy_with_logits over the edges of the seven classes, autograd's backward.  A yardstick, not a
comparison against this code.

  python tools/latreg_timing.py [--sizes 64 128 256] [--reps 10] [--warmup 2] [--out FILE.json]

Workloads: the distance to a sphere on lattices of n^3 vertices over [-1, 1]^3, perturbed by normal noise of a quarter of the spacing, all three terms on.
Before anything is timed the torch form must agree with the device within the accuracy rule of the tests, e <= 4 max(e_32, u G), with the torch form in float64 as the
reference and the torch form in float32 as e_32 - for the three terms and for the gradient; otherwise the case stops.
Candidates, alternating inside one process after the warm-up:
  value+grad        lr.value_and_grad(sdf)            the partial sums, the finishing workgroup, the gradient
  value             lr.value(sdf)                     the first two launches
  torch value+grad  the torch form and autograd's backward
  torch value       the torch form under no_grad
Two clocks per candidate: `call` is a host clock around one call that ends in a device synchronise (median of --reps calls, min - max); `queued` is device events around --reps
calls queued back to back, divided by --reps.
The byte floor: read sdf once, write grad once - 8 Nv bytes (4 Nv for the value alone) - at the 6.29 TB/s of a device copy (README)."""
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

COPY_RATE = 6.29e12          # bytes per second of a device copy (README)
U = 2.0 ** -24
CLASSES = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))
WEIGHTS = (1.0, 0.1, 0.1)
SIGN_SCALE = 10.0


def torch_terms(S, h, k):
    """S [nz, ny, nx] -> (eikonal, laplacian, sign) as 0-d tensors; no indexing by a mask, so nothing synchronises"""
    nz, ny, nx = S.shape
    c = lambda x, y, z: S[z:nz - 1 + z, y:ny - 1 + y, x:nx - 1 + x]
    gx = ((c(1, 0, 0) - c(0, 0, 0)) + (c(1, 1, 0) - c(0, 1, 0)) + (c(1, 0, 1) - c(0, 0, 1)) + (c(1, 1, 1) - c(0, 1, 1))) / (4 * h[0])
    gy = ((c(0, 1, 0) - c(0, 0, 0)) + (c(1, 1, 0) - c(1, 0, 0)) + (c(0, 1, 1) - c(0, 0, 1)) + (c(1, 1, 1) - c(1, 0, 1))) / (4 * h[1])
    gz = ((c(0, 0, 1) - c(0, 0, 0)) + (c(1, 0, 1) - c(1, 0, 0)) + (c(0, 1, 1) - c(0, 1, 0)) + (c(1, 1, 1) - c(1, 1, 0))) / (4 * h[2])
    eik = ((gx * gx + gy * gy + gz * gz).sqrt() - 1).square().mean()
    r = F.pad(((S[:, :, :-2] - S[:, :, 1:-1]) + (S[:, :, 2:] - S[:, :, 1:-1])) / h[0] ** 2, (1, 1))
    r = r + F.pad(((S[:, :-2] - S[:, 1:-1]) + (S[:, 2:] - S[:, 1:-1])) / h[1] ** 2, (0, 0, 1, 1))
    r = r + F.pad(((S[:-2] - S[1:-1]) + (S[2:] - S[1:-1])) / h[2] ** 2, (0, 0, 0, 0, 1, 1))
    lap = r.square().mean()
    total, V = 0, 0
    for dx, dy, dz in CLASSES:
        A, B = S[:nz - dz, :ny - dy, :nx - dx], S[dz:, dy:, dx:]
        yA, yB = (A >= 0).to(S.dtype), (B >= 0).to(S.dtype)
        cross = yA != yB
        both = F.binary_cross_entropy_with_logits(k * A, yB, reduction="none") + F.binary_cross_entropy_with_logits(k * B, yA, reduction="none")
        total = total + (both * cross).sum()
        V = V + cross.sum()
    return eik, lap, total / V.clamp(min=1)


def torch_loss(S, h, k, w):
    e, l, s = torch_terms(S, h, k)
    return w[0] * e + w[1] * l + w[2] * s


def clocks(cands, reps, warmup):
    t = {k: [] for k, _ in cands}
    for k in range(warmup + reps):
        for key, fn in cands:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if k >= warmup:
                t[key].append(1e3 * (time.perf_counter() - t0))
    out = {}
    for key, fn in cands:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        a = np.asarray(t[key])
        out[key] = {"call_median_ms": float(np.median(a)), "call_min_ms": float(a.min()), "call_max_ms": float(a.max()), "queued_ms": e0.elapsed_time(e1) / reps}
    return out


def ratio(dev, f32, f64):
    dev, f32, f64 = (x.detach().double() for x in (dev, f32, f64))
    e_gpu, e_32, G = float((dev - f64).abs().max()), float((f32 - f64).abs().max()), float(f64.abs().max())
    yard = max(e_32, U * G)
    return 0.0 if e_gpu == 0 else e_gpu / yard if yard > 0 else float("inf")


def measure(name, shape, sdf, h, reps, warmup):
    nx, ny, nz = shape
    lr = psdr.LatticeRegularizer(shape, h, weights=WEIGHTS, sign_scale=SIGN_SCALE)
    loss, grad = lr.value_and_grad(sdf)
    terms = lr.terms.clone()
    # the yardstick agrees with the device before it is timed
    refs = {}
    for dtype in (torch.float32, torch.float64):
        s = sdf.to(dtype).reshape(nz, ny, nx).requires_grad_()
        t = torch_terms(s, h, SIGN_SCALE)
        (WEIGHTS[0] * t[0] + WEIGHTS[1] * t[1] + WEIGHTS[2] * t[2]).backward()
        refs[dtype] = (torch.stack([x.detach() for x in t]), s.grad.reshape(-1))
        del s, t
    agree = {"eikonal": ratio(terms[0], refs[torch.float32][0][0], refs[torch.float64][0][0]), "laplacian": ratio(terms[1], refs[torch.float32][0][1], refs[torch.float64][0][1]),
             "sign": ratio(terms[2], refs[torch.float32][0][2], refs[torch.float64][0][2]), "grad": ratio(grad, refs[torch.float32][1], refs[torch.float64][1])}
    print("%s: shape %s, V = %d, e / max(e_32, u G) against the torch form: %s" % (name, shape, int(lr.num_crossings.cpu()[0]), ", ".join("%s %.2f" % kv for kv in agree.items())))
    if max(agree.values()) > 4.0:
        raise SystemExit("%s: the torch form and the device disagree: nothing timed" % name)
    del refs
    torch.cuda.empty_cache()
    ls = sdf.clone().reshape(nz, ny, nx).requires_grad_()

    def theirs():
        ls.grad = None
        torch_loss(ls, h, SIGN_SCALE, WEIGHTS).backward()

    def theirs_value():
        with torch.no_grad():
            torch_loss(ls, h, SIGN_SCALE, WEIGHTS)

    res = clocks([("value+grad", lambda: lr.value_and_grad(sdf)), ("value", lambda: lr.value(sdf)), ("torch value+grad", theirs), ("torch value", theirs_value)], reps, warmup)
    nv = lr.num_lattice
    floors = {"value+grad": 1e3 * 8.0 * nv / COPY_RATE, "value": 1e3 * 4.0 * nv / COPY_RATE}
    res.update({"case": name, "shape": list(shape), "agreement": agree, "reps": reps, "warmup": warmup, "floor_ms": floors, "plan": list(psdr.launch_plan_lr(shape)),
                "weights": list(WEIGHTS), "sign_scale": SIGN_SCALE})
    for key in ("value+grad", "value", "torch value+grad", "torch value"):
        r = res[key]
        print("  %-17s call %10.4f ms [%10.4f, %10.4f]   queued %10.4f ms" % (key, r["call_median_ms"], r["call_min_ms"], r["call_max_ms"], r["queued_ms"]))
    for key in ("value+grad", "value"):
        res["%s: torch / ours (call)" % key] = res["torch " + key]["call_median_ms"] / res[key]["call_median_ms"]
        res["%s: torch / ours (queued)" % key] = res["torch " + key]["queued_ms"] / res[key]["queued_ms"]
        res["%s: over the byte floor (queued)" % key] = res[key]["queued_ms"] / floors[key]
        print("  %-17s torch / ours %.1f per call, %.1f queued; byte floor %.4f ms, ours at %.1f x" % (key, res["%s: torch / ours (call)" % key], res["%s: torch / ours (queued)" % key],
              floors[key], res["%s: over the byte floor (queued)" % key]), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("latreg_timing.py measures on the GPU: none visible")
    res = []
    for n in opt.sizes:
        shape = (n, n, n)
        h = psdr.lattice_spacing(shape, -1.0, 1.0)
        pos = psdr.lattice_points(shape, -1.0, 1.0).cuda()
        noise = torch.from_numpy(np.random.default_rng(n).normal(0.0, 0.25 * h[0], len(pos))).cuda()
        sdf = ((pos.double() - torch.tensor([0.031, -0.047, 0.052], device="cuda", dtype=torch.float64)).norm(dim=1).sub(0.642) + noise).float()
        del pos, noise
        res.append(measure("sphere %d^3" % n, shape, sdf, h, opt.reps, opt.warmup))
    print(json.dumps(res))
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
