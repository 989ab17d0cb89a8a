"""The point-to-mesh distance, value plus both gradients (psdr.PointMeshDistance.value_and_grad), against the same loss written with torch ops only - what a user could do
before it existed.  A yardstick, not a comparison against this code.

  python tools/pointmesh_timing.py [--reps 10] [--warmup 2] [--out FILE.json] [--skip-largest]

Workloads, weights (1, 1), squared: bunny_low.obj's jittered vertices (2 503) against the bunny (4 968 faces); 20 000 points sampled from a displaced bunny against the
bunny; 20 000 points sampled from the config-5 blob (scenes.icosphere(6): 40 962 vertices, 81 920 faces) against the blob; the blob's 40 962 jittered vertices against it.
Candidates, alternating inside one process after the warm-up:
  fused       pm.value_and_grad(points, v)                two scans, two stable sorts, four launches of the evaluation
  torch       the cascade as torch.where over [chunk, F] blocks under no_grad with a running minimum for the faces' direction (chunk: the block's temporaries, counted as
              60 floats per pair, stay under --block-bytes, default 2 GB), then the loss through index_select with the winners' barycentrics as constants and
              .backward() with points and v as leaves, whose index_add_ scatters with float atomics.
Two clocks per candidate: `call` is a host clock around one call that ends in a device synchronise (median of --reps calls, min - max); `queued` is device events around
--reps calls queued back to back, divided by --reps: what the stream is busy for when nothing waits.  The two scans alone are timed the same way.
The scans' floor: pairs x VALU instructions per (query, candidate) pair / the device's lane-issue rate.  VALU_PER_PAIR is counted in the inner loop of the compiled
k_scan<2, false> and k_scan<2, true> (hipcc -S --cuda-device-only: the vector instructions of the loop body, which serves 4 candidates x 2 queries; both scans hold the
same count); the lane-issue rate is 256 CUs x 4 SIMDs x 32 lanes per clock at 2.4 GHz = 78.6e12 lane-instructions per second, as in tools/chamfer_timing.py.  Both
directions are scanned, so pairs = 2 N F.  The table also gives the share of face indices on which the two forms differ, the relative l2 distance of the gradients and
whether ten fused gradients agree bit for bit."""
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

VALU_PER_PAIR = 1053.0 / 8.0        # k_scan<2, .>: 1053 vector instructions in the inner loop's body, which serves 4 candidates x 2 queries
LANE_RATE = 256 * 4 * 32 * 2.4e9        # lane-instructions per second
CONFIG5_STEP_MS = 238.878               # config5.api.step_ms.reverse_vertices of the committed BENCH_r06.json: quoted, not re-measured
FLOATS_PER_PAIR = 60                    # the temporaries of one block of the torch cascade, counted generously


def _dot(x, y):
    return (x * y).sum(-1)


def _quot(num, den):
    zero = den == 0
    return torch.where(zero, torch.zeros_like(num), num / torch.where(zero, torch.ones_like(den), den))


def torch_pairs(P, A, B, C):
    """the cascade on broadcastable [..., 3] tensors -> (s, t, dist2)"""
    ab, ac, ap, bp, cp = B - A, C - A, P - A, P - B, P - C
    d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    d43, d56 = d4 - d3, d5 - d6
    den = va + vb + vc
    s, t = _quot(vb, den), _quot(vc, den)
    zero, one = torch.zeros_like(s), torch.ones_like(s)
    t6 = _quot(d43, d43 + d56)
    for cond, rs, rt in (((va <= 0) & (d43 >= 0) & (d56 >= 0), one - t6, t6), ((vb <= 0) & (d2 >= 0) & (d6 <= 0), zero, _quot(d2, d2 - d6)),
                         ((d6 >= 0) & (d5 <= d6), zero, one), ((vc <= 0) & (d1 >= 0) & (d3 <= 0), _quot(d1, d1 - d3), zero),
                         ((d3 >= 0) & (d4 <= d3), one, zero), ((d1 <= 0) & (d2 <= 0), zero, zero)):
        s, t = torch.where(cond, rs, s), torch.where(cond, rt, t)
    e = ap - (s.unsqueeze(-1) * ab + t.unsqueeze(-1) * ac)
    return s, t, _dot(e, e)


def torch_indices(p, v, faces, rows):
    """(face_of_point, bary_p, point_of_face, bary_f) by chunks of `rows` points, no autograd"""
    with torch.no_grad():
        A, B, C = (v[faces[:, k]].unsqueeze(0) for k in range(3))
        N, F = len(p), len(faces)
        a = torch.empty(N, dtype=torch.int64, device=p.device)
        st_p = torch.empty((N, 2), device=p.device)
        best = torch.full((F,), float("inf"), device=p.device)
        b = torch.zeros(F, dtype=torch.int64, device=p.device)
        st_f = torch.zeros((F, 2), device=p.device)
        cols = torch.arange(F, device=p.device)
        for r in range(0, N, rows):
            s, t, d = torch_pairs(p[r:r + rows].unsqueeze(1), A, B, C)
            k = d.argmin(1)
            at = torch.arange(len(k), device=p.device)
            a[r:r + rows] = k
            st_p[r:r + rows] = torch.stack([s[at, k], t[at, k]], 1)
            val, k = d.min(0)
            better = val < best
            best = torch.where(better, val, best)
            b = torch.where(better, k + r, b)
            st_f = torch.where(better.unsqueeze(1), torch.stack([s[k, cols], t[k, cols]], 1), st_f)
    bary = lambda st: torch.stack([1 - st[:, 0] - st[:, 1], st[:, 0], st[:, 1]], 1)
    return a, bary(st_p), b, bary(st_f)


def torch_loss(p, v, faces, rows):
    a, bary_p, b, bary_f = torch_indices(p.detach(), v.detach(), faces, rows)
    q_p = (bary_p.unsqueeze(-1) * v.index_select(0, faces.index_select(0, a).reshape(-1)).reshape(-1, 3, 3)).sum(1)
    q_f = (bary_f.unsqueeze(-1) * v.index_select(0, faces.reshape(-1)).reshape(-1, 3, 3)).sum(1)
    return ((p - q_p) ** 2).sum(1).mean() + ((p.index_select(0, b) - q_f) ** 2).sum(1).mean(), a


def measure(name, p_np, v_np, f_np, reps, warmup, block_bytes, step_ms):
    N, F = len(p_np), len(f_np)
    pm = psdr.PointMeshDistance(f_np, len(v_np))
    p, v = torch.from_numpy(np.ascontiguousarray(p_np, np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(v_np, np.float32)).cuda()
    faces = torch.from_numpy(np.ascontiguousarray(f_np, np.int64)).cuda()
    faces32 = faces.to(torch.int32)
    lp, lv = p.clone().requires_grad_(), v.clone().requires_grad_()
    rows = max(1, int(block_bytes // (4 * FLOATS_PER_PAIR * F)))
    index_torch = {}

    def fused():
        return pm.value_and_grad(p, v)

    def torch_ops():
        lp.grad = lv.grad = None
        loss, a = torch_loss(lp, lv, faces, rows)
        loss.backward()
        index_torch["a"] = a
        return loss.detach(), lp.grad, lv.grad

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
    # the two scans alone, for the floor
    from psdr_jit_amd import pointmesh as pmod
    scan_ms = []
    for direction in (0, 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        pmod._scan(p, v, faces32, direction, p.device)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            pmod._scan(p, v, faces32, direction, p.device)
        e1.record()
        torch.cuda.synchronize()
        scan_ms.append(e0.elapsed_time(e1) / reps)
    scans = sum(scan_ms)
    stable = all(torch.equal(fused()[1], last["fused"][1]) and torch.equal(fused()[2], last["fused"][2]) for _ in range(10))
    fused()
    floor_ms = 1e3 * 2.0 * N * F * VALU_PER_PAIR / LANE_RATE
    rel = lambda k: float((last["fused"][k].double() - last["torch"][k].double()).norm() / last["torch"][k].double().norm())
    res = {"case": name, "points": N, "faces": F, "chunk_rows": rows, "reps": reps, "warmup": warmup,
           "plan_points": list(psdr.launch_plan_pm(N, F)), "plan_faces": list(psdr.launch_plan_pm(F, N)),
           "scan_points_queued_ms": scan_ms[0], "scan_faces_queued_ms": scan_ms[1], "scans_queued_ms": scans, "floor_ms": floor_ms, "scans_over_floor": scans / floor_ms,
           "valu_per_pair": VALU_PER_PAIR, "fused_bit_stable_over_10_runs": bool(stable),
           "loss": {key: float(last[key][0]) for key, _ in cands},
           "index_disagreement_torch_vs_fused": float((index_torch["a"] != pm.nearest[0].long()).float().mean()),
           "rel_l2_dpoints_vs_torch": rel(1), "rel_l2_dv_vs_torch": rel(2)}
    print("%s: N = %d, F = %d, torch chunk %d rows" % (name, N, F, rows))
    for key, _ in cands:
        a = np.asarray(t[key])
        res[key] = {"call_median_ms": float(np.median(a)), "call_min_ms": float(a.min()), "call_max_ms": float(a.max()), "queued_ms": queued[key]}
        print("  %-6s call %10.4f ms [%10.4f, %10.4f]   queued %10.4f ms" % (key, np.median(a), a.min(), a.max(), queued[key]))
    res["torch_over_fused_queued"] = queued["torch"] / queued["fused"]
    res["torch_over_fused_call"] = res["torch"]["call_median_ms"] / res["fused"]["call_median_ms"]
    res["share_of_config5_step"] = queued["fused"] / step_ms
    print("  torch / fused: %.1f queued, %.1f per call; scans %.4f + %.4f ms, floor %.4f ms (%.2f x); loss fused %.9g torch %.9g; indices that differ %.2e; "
          "rel l2 d/dpoints %.2e d/dv %.2e; bit-stable %s; %.3f %% of the config-5 step"
          % (res["torch_over_fused_queued"], res["torch_over_fused_call"], scan_ms[0], scan_ms[1], floor_ms, scans / floor_ms, res["loss"]["fused"], res["loss"]["torch"],
             res["index_disagreement_torch_vs_fused"], res["rel_l2_dpoints_vs_torch"], res["rel_l2_dv_vs_torch"], stable, 100.0 * res["share_of_config5_step"]), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--block-bytes", type=float, default=2e9)
    ap.add_argument("--out", default="")
    ap.add_argument("--skip-largest", action="store_true")
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pointmesh_timing.py measures on the GPU: none visible")
    step_ms = CONFIG5_STEP_MS
    rng = np.random.default_rng(0)
    jitter = lambda v: (v + rng.normal(0.0, 0.01, v.shape)).astype(np.float32)
    bf, _bn, bv, _ft, _vt = subdiv_ref.load_obj(subdiv_ref.BUNNY)
    bf, bv = np.asarray(bf).reshape(-1, 3), ((bv - bv.min(0)) / (bv.max(0) - bv.min(0)).max()).astype(np.float32)
    args = (opt.reps, opt.warmup, opt.block_bytes, step_ms)
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
