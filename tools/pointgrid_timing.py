"""The grid search against the scan (psdr.nearest_points / psdr.ChamferDistance with search="grid" and "scan"), both in one process, alternating after the warm-up.

  python tools/pointgrid_timing.py [--reps 10] [--warmup 2] [--out FILE.json] [--skip-largest]

Workloads, N = M each: bunny_low.obj's vertices against a jittered copy (2 503); 20 000 points sampled from the bunny against 20 000 sampled from a displaced bunny; the
config-5 blob's vertices (scenes.icosphere(6): 40 962) against a jittered copy; its one-level Loop subdivision (163 842) likewise; 10^6 points sampled from the bunny
against 10^6 from the displaced bunny.  weights (1, 1), squared.  Per workload:
  cd          cd.value_and_grad(x, y): scan, grid (both grids built in the call), and grid with y_grid=PointGrid(y) built before (a fixed target)
  search      nearest_points(x, y) alone: scan, grid search of a prebuilt grid, and the build alone - the saving of a reused PointGrid is the build
Two clocks: `call` is a host clock around one call that ends in a device synchronise (median of --reps calls, min - max); `queued` is device events around --reps calls
queued back to back, divided by --reps: what the stream is busy for when nothing waits.  Then the pairs tested per query against m, the fallback's share (both from the
device's statistics) and whether the grid's arrays equal the scan's bit for bit.  The crossover is read from the table: the smallest size at which grid beats scan."""
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


def clocks(cands, reps, warmup):
    """{name: {"call_median_ms", "call_min_ms", "call_max_ms", "queued_ms"}}; the candidates alternate inside every repetition"""
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


def measure(name, x_np, y_np, reps, warmup):
    n, m = len(x_np), len(y_np)
    x, y = torch.from_numpy(np.ascontiguousarray(x_np, np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(y_np, np.float32)).cuda()
    scan, grid = psdr.ChamferDistance(), psdr.ChamferDistance(search="grid")
    yg = psdr.PointGrid(y)
    cd = clocks([("scan", lambda: scan.value_and_grad(x, y)), ("grid", lambda: grid.value_and_grad(x, y)), ("grid_reused", lambda: grid.value_and_grad(x, y, y_grid=yg))], reps, warmup)
    search = clocks([("scan", lambda: psdr.nearest_points(x, y)), ("grid_search", lambda: psdr.nearest_points(x, yg)), ("grid_build", lambda: psdr.PointGrid(y))], reps, warmup)
    gi, gd, stats = psdr.nearest_points(x, yg, return_stats=True)
    si, sd = psdr.nearest_points(x, y)
    same = bool(torch.equal(gi, si) and torch.equal(gd.view(torch.int32), sd.view(torch.int32)))
    a, b = scan.value_and_grad(x, y), grid.value_and_grad(x, y)
    same_cd = all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(a, b))
    fallback, pairs = (int(v) for v in stats.cpu())
    p = psdr.grid_plan(n, m)
    res = {"case": name, "n": n, "m": m, "res": p.res, "reps": reps, "warmup": warmup, "cd": cd, "search": search, "pairs_per_query": pairs / n, "pairs_share_of_m": pairs / n / m,
           "fallback_queries": fallback, "fallback_share": fallback / n, "grid_equals_scan_bits": same, "cd_equals_scan_bits": bool(same_cd),
           "scan_over_grid_cd_queued": cd["scan"]["queued_ms"] / cd["grid"]["queued_ms"], "scan_over_grid_search_queued": search["scan"]["queued_ms"] / search["grid_search"]["queued_ms"]}
    print("%s: N = M = %d, res %d" % (name, n, p.res))
    for part, table in (("cd", cd), ("search", search)):
        for key, v in table.items():
            print("  %-6s %-12s call %10.4f ms [%10.4f, %10.4f]   queued %10.4f ms" % (part, key, v["call_median_ms"], v["call_min_ms"], v["call_max_ms"], v["queued_ms"]))
    print("  pairs per query %.1f (%.3g of m), fallback %d (%.3g of n); scan / grid queued: cd %.2f, search alone %.2f; bits equal: search %s, cd %s"
          % (res["pairs_per_query"], res["pairs_share_of_m"], fallback, res["fallback_share"], res["scan_over_grid_cd_queued"], res["scan_over_grid_search_queued"], same, same_cd), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    ap.add_argument("--skip-largest", action="store_true")
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pointgrid_timing.py measures on the GPU: none visible")
    rng = np.random.default_rng(0)
    jitter = lambda v: (v + rng.normal(0.0, 0.01, v.shape)).astype(np.float32)
    bf, _bn, bv, _ft, _vt = subdiv_ref.load_obj(subdiv_ref.BUNNY)
    bf, bv = np.asarray(bf).reshape(-1, 3), ((bv - bv.min(0)) / (bv.max(0) - bv.min(0)).max()).astype(np.float32)
    moved = (bv + 0.05 * np.sin(3.0 * bv[:, [1, 2, 0]])).astype(np.float32)

    def sampled(count):
        sa, sb = psdr.SurfaceSampler(bf, len(bv), num_points=count, seed=0).resample(bv), psdr.SurfaceSampler(bf, len(bv), num_points=count, seed=1).resample(moved)
        return sa(torch.from_numpy(bv)).cpu().numpy(), sb(torch.from_numpy(moved)).cpu().numpy()

    res = [measure("bunny_low.obj vertices", bv, jitter(bv), opt.reps, opt.warmup)]
    res.append(measure("20 000 sampled points", *sampled(20000), opt.reps, opt.warmup))
    v, f = scenes.icosphere(6, radius=150.0, noise=0.01, seed=0)
    v, f = np.asarray(v, np.float32).reshape(-1, 3) / 150.0, np.asarray(f).reshape(-1, 3)
    res.append(measure("config-5 blob", v, jitter(v), opt.reps, opt.warmup))
    sub = psdr.Subdivision(f, v.shape[0], levels=1)
    fine = sub.refine(torch.from_numpy(v)).cpu().numpy()
    res.append(measure("config-5 blob, one Loop level", fine, jitter(fine), max(3, opt.reps // 2), 1))
    if not opt.skip_largest:
        res.append(measure("10^6 sampled points", *sampled(10 ** 6), 3, 1))
    beats = [r["n"] for r in res if r["scan_over_grid_cd_queued"] > 1.0]
    print("crossover: the smallest measured size at which cd with the grid beats the scan (queued): %s" % (min(beats) if beats else "none"))
    print(json.dumps(res))
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
