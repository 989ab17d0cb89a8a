"""The Chamfer distance, value plus both gradients (psdr.ChamferDistance.value_and_grad), against the same loss written with torch ops only - what a user could do before
it existed.  A yardstick, not a comparison against this code.

  python tools/chamfer_timing.py [--reps 10] [--warmup 2] [--out FILE.json]

Workloads, N = M each: bunny_low.obj's vertices against a jittered copy (2 503); 20 000 points sampled from the bunny against 20 000 sampled from a displaced bunny; the
config-5 blob's vertices (scenes.icosphere(6): 40 962) against a jittered copy; its one-level Loop subdivision (163 842) likewise.  weights (1, 1), squared.  Candidates,
alternating inside one process after the warm-up:
  fused       cd.value_and_grad(x, y)                     two scans, two stable sorts, three launches of the evaluation
  torch       "cdist": torch.cdist(x, y) -> min over both axes -> .backward() with x and y leaves: the N x M matrix exists (4 N M bytes, and again in the backward); the
              expansion form.  Used where 4 N M bytes <= --matrix-bytes (default 16 GB).
              "chunked": the indices from torch.cdist on row chunks of at most --matrix-bytes / 8 under no_grad (a running minimum over the chunks for the other axis),
              then the loss through index_select and .backward(), whose scatter uses float atomics.  Used where the matrix does not fit.
Two clocks per candidate: `call` is a host clock around one call that ends in a device synchronise (median of --reps calls, min - max); `queued` is device events around
--reps calls queued back to back, divided by --reps: what the stream is busy for when nothing waits.
The scan's floor: pairs x VALU instructions per (query, candidate) pair / the device's lane-issue rate.  VALU_PER_PAIR is counted in the inner loop of the compiled
k_scan<4> (llvm-objdump -d on the unit's code object: the vector instructions between two LDS reads of a plane, divided by the 16 pairs they serve); the lane-issue rate
is 256 CUs x 4 SIMDs x 32 lanes per clock at 2.4 GHz = 78.6e12 lane-instructions per second (a wave64 vector instruction takes 2 cycles on a SIMD).  Both directions are
scanned, so pairs = 2 N M.  The table also gives the share of index disagreements between the two forms and whether ten fused gradients agree bit for bit."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import psdr_jit_amd as psdr
import scenes
import subdiv_ref

VALU_PER_PAIR = 181.0 / 16.0        # k_scan<4>: 181 vector instructions per LDS read of the three planes, which serves 4 candidates x 4 queries
LANE_RATE = 256 * 4 * 32 * 2.4e9        # lane-instructions per second


def torch_cdist(x, y):
    d = torch.cdist(x, y)
    return (d.min(1).values ** 2).mean() + (d.min(0).values ** 2).mean()


def torch_indices(x, y, rows):
    """(a, b) by chunks of `rows` rows of the distance matrix, no autograd"""
    with torch.no_grad():
        a = torch.empty(len(x), dtype=torch.int64, device=x.device)
        best = torch.full((len(y),), float("inf"), device=x.device)
        b = torch.zeros(len(y), dtype=torch.int64, device=x.device)
        for r in range(0, len(x), rows):
            d = torch.cdist(x[r:r + rows], y)
            a[r:r + rows] = d.argmin(1)
            v, k = d.min(0)
            better = v < best
            best = torch.where(better, v, best)
            b = torch.where(better, k + r, b)
    return a, b


def torch_chunked(x, y, rows):
    a, b = torch_indices(x, y, rows)
    return ((x - y.index_select(0, a)) ** 2).sum(1).mean() + ((y - x.index_select(0, b)) ** 2).sum(1).mean()


def measure(name, x_np, y_np, reps, warmup, matrix_bytes):
    n, m = len(x_np), len(y_np)
    cd = psdr.ChamferDistance()
    x, y = torch.from_numpy(np.ascontiguousarray(x_np, np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(y_np, np.float32)).cuda()
    lx, ly = x.clone().requires_grad_(), y.clone().requires_grad_()
    form = "cdist" if 4 * n * m <= matrix_bytes else "chunked"
    rows = max(1, int(matrix_bytes // 8 // (4 * m)))

    def fused():
        return cd.value_and_grad(x, y)

    def torch_ops():
        lx.grad = ly.grad = None
        loss = torch_cdist(lx, ly) if form == "cdist" else torch_chunked(lx, ly, rows)
        loss.backward()
        return loss.detach(), lx.grad, ly.grad

    cands = [("fused", fused), ("torch", torch_ops)]
    t, last = {k: [] for k, _ in cands}, {}
    for k in range(warmup + reps):
        for key, fn in cands:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            if k >= warmup:
                t[key].append(1e3 * (time.perf_counter() - t0))
            last[key] = tuple(o.clone() for o in out)
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
    # the scans alone, for the floor
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        psdr.nearest_points(x, y)
        psdr.nearest_points(y, x)
    e1.record()
    torch.cuda.synchronize()
    scans = e0.elapsed_time(e1) / reps
    stable = all(torch.equal(fused()[1], last["fused"][1]) and torch.equal(fused()[2], last["fused"][2]) for _ in range(10))
    a_t, _b_t = torch_indices(x, y, rows)
    floor_ms = 1e3 * 2.0 * n * m * VALU_PER_PAIR / LANE_RATE
    res = {"case": name, "n": n, "m": m, "torch_form": form, "chunk_rows": rows if form == "chunked" else None, "reps": reps, "warmup": warmup,
           "plan_xy": list(psdr.launch_plan(n, m)), "scans_queued_ms": scans, "floor_ms": floor_ms, "scans_over_floor": scans / floor_ms,
           "valu_per_pair": VALU_PER_PAIR, "fused_bit_stable_over_10_runs": bool(stable),
           "loss": {key: float(last[key][0]) for key, _ in cands},
           "index_disagreement_torch_vs_fused": float((a_t != cd.nearest[0].long()).float().mean()),
           "rel_l2_dx_vs_torch": float((last["fused"][1].double() - last["torch"][1].double()).norm() / last["torch"][1].double().norm())}
    print("%s: N = M = %d, torch form: %s" % (name, n, form))
    for key, _ in cands:
        a = np.asarray(t[key])
        res[key] = {"call_median_ms": float(np.median(a)), "call_min_ms": float(a.min()), "call_max_ms": float(a.max()), "queued_ms": queued[key]}
        print("  %-6s call %10.4f ms [%10.4f, %10.4f]   queued %10.4f ms" % (key, np.median(a), a.min(), a.max(), queued[key]))
    res["torch_over_fused_queued"] = queued["torch"] / queued["fused"]
    res["torch_over_fused_call"] = res["torch"]["call_median_ms"] / res["fused"]["call_median_ms"]
    print("  torch / fused: %.1f queued, %.1f per call; the two scans %.4f ms, floor %.4f ms (%.2f x); loss fused %.9g torch %.9g; indices that differ %.2e; dx rel l2 %.2e; bit-stable %s"
          % (res["torch_over_fused_queued"], res["torch_over_fused_call"], scans, floor_ms, scans / floor_ms, res["loss"]["fused"], res["loss"]["torch"],
             res["index_disagreement_torch_vs_fused"], res["rel_l2_dx_vs_torch"], stable), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--matrix-bytes", type=float, default=16e9)
    ap.add_argument("--out", default="")
    ap.add_argument("--skip-largest", action="store_true")
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("chamfer_timing.py measures on the GPU: none visible")
    rng = np.random.default_rng(0)
    jitter = lambda v: (v + rng.normal(0.0, 0.01, v.shape)).astype(np.float32)
    bf, _bn, bv, _ft, _vt = subdiv_ref.load_obj(subdiv_ref.BUNNY)
    bf, bv = np.asarray(bf).reshape(-1, 3), ((bv - bv.min(0)) / (bv.max(0) - bv.min(0)).max()).astype(np.float32)
    res = [measure("bunny_low.obj vertices", bv, jitter(bv), opt.reps, opt.warmup, opt.matrix_bytes)]
    moved = (bv + 0.05 * np.sin(3.0 * bv[:, [1, 2, 0]])).astype(np.float32)
    sa, sb = psdr.SurfaceSampler(bf, len(bv), num_points=20000, seed=0).resample(bv), psdr.SurfaceSampler(bf, len(bv), num_points=20000, seed=1).resample(moved)
    res.append(measure("20 000 sampled points", sa(torch.from_numpy(bv)).cpu().numpy(), sb(torch.from_numpy(moved)).cpu().numpy(), opt.reps, opt.warmup, opt.matrix_bytes))
    v, f = scenes.icosphere(6, radius=150.0, noise=0.01, seed=0)
    v, f = np.asarray(v, np.float32).reshape(-1, 3) / 150.0, np.asarray(f).reshape(-1, 3)
    res.append(measure("config-5 blob", v, jitter(v), opt.reps, opt.warmup, opt.matrix_bytes))
    if not opt.skip_largest:
        sub = psdr.Subdivision(f, v.shape[0], levels=1)
        fine = sub.refine(torch.from_numpy(v)).cpu().numpy()
        res.append(measure("config-5 blob, one Loop level", fine, jitter(fine), max(2, opt.reps // 3), 1, opt.matrix_bytes))
    print(json.dumps(res))
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
