"""The signed distance (psdr.winding_number, psdr.signed_distance, psdr.SignedDistance plus its backward) against the same definition written with torch ops only - what a
user could do before it existed - and against closest_points_on_mesh in the same process.  A yardstick, not a comparison against this code.

  python tools/sdf_timing.py [--reps 30] [--warmup 2] [--out FILE.json] [--skip-largest]

Workloads, the four sizes of tools/pointmesh_timing.py: bunny_low.obj's jittered vertices (2 503) against the bunny (4 968 faces); 20 000 points sampled from a displaced bunny
against the bunny; 20 000 points sampled from the config-5 blob (scenes.icosphere(6): 40 962 vertices, 81 920 faces) against the blob; the blob's 40 962 jittered vertices
against it.
Candidates, alternating inside one process after the warm-up:
  winding     psdr.winding_number(points, v, faces)          the record kernel, the scan, the merge (faces already on the GPU)
  signed      psdr.signed_distance(points, v, faces)         closest_points_on_mesh's scan, then the above with the sign
  sd+backward sd(points, v).backward(g)                      the above, a stable sort and the three launches of the vector-Jacobian product
  nearest     psdr.closest_points_on_mesh(points, v, faces)  the point-to-mesh scan alone
  torch       the winding number as torch ops over [chunk, F] blocks under no_grad (chunk: the block's temporaries, counted as 40 floats per pair, stay under --block-bytes,
              default 2 GB), summed over the faces per block
Two clocks per candidate: `call` is a host clock around one call that ends in a device synchronise (median of --reps calls, min - max); `queued` is device events around --reps
calls queued back to back, divided by --reps: what the stream is busy for when nothing waits.
The scan's floor: N F pairs x VALU instructions per pair / the device's lane-issue rate.  VALU_PER_PAIR is counted in the inner loop of the compiled k_scan<2> (hipcc -S
--cuda-device-only: the vector instructions of the loop body, which serves 1 face x 2 points); the lane-issue rate is 256 CUs x 4 SIMDs x 32 lanes per clock at 2.4 GHz = 78.6e12
lane-instructions per second, as in tools/pointmesh_timing.py.  The table also gives the largest deviation of w from the torch form and the share of points on which the two
signs differ."""
import argparse
import json
import math
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

VALU_PER_PAIR = 301.0 / 2.0             # k_scan<2>: 301 vector instructions in the inner loop's body, which serves 1 face x 2 points
LANE_RATE = 256 * 4 * 32 * 2.4e9        # lane-instructions per second
FLOATS_PER_PAIR = 40                    # the temporaries of one block of the torch form, counted generously


def _dot(x, y):
    return (x * y).sum(-1)


def torch_winding(p, v, faces, rows):
    """the definition by chunks of `rows` points, no autograd"""
    with torch.no_grad():
        A, B, C = (v[faces[:, k]].unsqueeze(0) for k in range(3))
        w = torch.empty(len(p), device=p.device)
        for r in range(0, len(p), rows):
            P = p[r:r + rows].unsqueeze(1)
            a, b, c = A - P, B - P, C - P
            la, lb, lc = a.norm(dim=-1), b.norm(dim=-1), c.norm(dim=-1)
            nm = _dot(a, torch.linalg.cross(b, c, dim=-1))
            dn = la * lb * lc + _dot(a, b) * lc + _dot(b, c) * la + _dot(c, a) * lb
            th = torch.where(nm == 0, torch.zeros_like(nm), torch.atan2(nm, dn))
            w[r:r + rows] = th.sum(1) / (2.0 * math.pi)
    return w


def measure(name, p_np, v_np, f_np, reps, warmup, block_bytes):
    N, F = len(p_np), len(f_np)
    sd = psdr.SignedDistance(f_np, len(v_np))
    p, v = torch.from_numpy(np.ascontiguousarray(p_np, np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(v_np, np.float32)).cuda()
    faces = torch.from_numpy(np.ascontiguousarray(f_np, np.int64)).cuda()
    faces32 = faces.to(torch.int32)
    g = torch.from_numpy(np.random.default_rng(3).uniform(-1.0, 1.0, N).astype(np.float32)).cuda()
    lp, lv = p.clone().requires_grad_(), v.clone().requires_grad_()
    rows = max(1, int(block_bytes // (4 * FLOATS_PER_PAIR * F)))

    def backward():
        lp.grad = lv.grad = None
        s = sd(lp, lv)
        s.backward(g)
        return s.detach(), lp.grad, lv.grad

    cands = [("winding", lambda: (psdr.winding_number(p, v, faces32),)), ("signed", lambda: tuple(psdr.signed_distance(p, v, faces32))), ("sd+backward", backward),
             ("nearest", lambda: psdr.closest_points_on_mesh(p, v, faces32)), ("torch", lambda: (torch_winding(p, v, faces, rows),))]
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
    stable = all(all(torch.equal(a, b) for a, b in zip(backward(), last["sd+backward"])) for _ in range(10))
    floor_ms = 1e3 * float(N) * F * VALU_PER_PAIR / LANE_RATE
    w, wt = last["winding"][0], last["torch"][0]
    res = {"case": name, "points": N, "faces": F, "chunk_rows": rows, "reps": reps, "warmup": warmup, "plan": list(psdr.launch_plan_pm(N, F)),
           "floor_ms": floor_ms, "valu_per_pair": VALU_PER_PAIR, "winding_over_floor": queued["winding"] / floor_ms,
           "scan_share_of_signed": queued["winding"] / queued["signed"], "bit_stable_over_10_runs": bool(stable),
           "max_abs_w_minus_torch": float((w - wt).abs().max()), "signs_that_differ_from_torch": float(((w > 0.5) != (wt > 0.5)).float().mean()),
           "inside": float((w > 0.5).float().mean())}
    print("%s: N = %d, F = %d, plan %s, torch chunk %d rows" % (name, N, F, tuple(psdr.launch_plan_pm(N, F)), rows))
    for key, _ in cands:
        a = np.asarray(t[key])
        res[key] = {"call_median_ms": float(np.median(a)), "call_min_ms": float(a.min()), "call_max_ms": float(a.max()), "queued_ms": queued[key]}
        print("  %-12s call %10.4f ms [%10.4f, %10.4f]   queued %10.4f ms" % (key, np.median(a), a.min(), a.max(), queued[key]))
    res["torch_over_winding_queued"] = queued["torch"] / queued["winding"]
    res["torch_over_winding_call"] = res["torch"]["call_median_ms"] / res["winding"]["call_median_ms"]
    print("  torch / winding: %.1f queued, %.1f per call; floor %.4f ms (winding at %.2f x); max |w - torch| %.2e; signs that differ %.2e; inside %.3f; bit-stable %s"
          % (res["torch_over_winding_queued"], res["torch_over_winding_call"], floor_ms, res["winding_over_floor"], res["max_abs_w_minus_torch"],
             res["signs_that_differ_from_torch"], res["inside"], stable), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--block-bytes", type=float, default=2e9)
    ap.add_argument("--out", default="")
    ap.add_argument("--skip-largest", action="store_true")
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sdf_timing.py measures on the GPU: none visible")
    rng = np.random.default_rng(0)
    jitter = lambda v: (v + rng.normal(0.0, 0.01, v.shape)).astype(np.float32)
    bf, _bn, bv, _ft, _vt = subdiv_ref.load_obj(subdiv_ref.BUNNY)
    bf, bv = np.asarray(bf).reshape(-1, 3), ((bv - bv.min(0)) / (bv.max(0) - bv.min(0)).max()).astype(np.float32)
    args = (opt.reps, opt.warmup, opt.block_bytes)
    res = [measure("2 503 points, bunny", jitter(bv), bv, bf, *args)]
    moved = (bv + 0.05 * np.sin(3.0 * bv[:, [1, 2, 0]])).astype(np.float32)
    sample = lambda f, v, seed: psdr.SurfaceSampler(f, len(v), num_points=20000, seed=seed).resample(v)(torch.from_numpy(v)).cpu().numpy()
    res.append(measure("20 000 points, bunny", sample(bf, moved, 1), bv, bf, *args))
    v, f = scenes.icosphere(6, radius=150.0, noise=0.01, seed=0)
    v, f = np.asarray(v, np.float32).reshape(-1, 3) / 150.0, np.asarray(f).reshape(-1, 3)
    res.append(measure("20 000 points, config-5 blob", sample(f, (v * np.float32(1.03)).astype(np.float32), 2), v, f, *args))
    if not opt.skip_largest:
        res.append(measure("40 962 points, config-5 blob", jitter(v), v, f, *args))
    print(json.dumps(res))
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
