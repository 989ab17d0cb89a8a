"""The Laplacian preconditioner's solve (psdr_hip_precond_solve) against the same algorithm written with torch ops only - what a user could do before it existed.

  python tools/precond_timing.py [--level 6] [--lambda 19] [--rtol 1e-4] [--reps 30] [--warmup 5] [--out FILE.json]

Workload: the connectivity of the config-5 blob (scenes.icosphere(level): 40 962 vertices at level 6), M = I + lambda L, a seeded random right-hand side [n, 3].
Both forms are Jacobi-preconditioned conjugate gradients in float32 from x0 = 0 with per-column scalars kept on the device, and both look at the residual
recomputed from x after every 8 iterations (one small copy to the host, the only synchronisation) and go on from it.  The torch form multiplies with a
torch.sparse CSR matrix and guards its quotients with torch.where.  The two alternate inside one process after a warm-up; a solve is timed with a host clock
around the call and a device synchronise; the table gives the median and the min-max spread in ms, iterations and kernel launches per solve (the torch
form's launches are counted by the profiler in one extra solve outside the timed window)."""
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

CHUNK = 8
STEP_MS = 238.9          # config5.api.step_ms.reverse_vertices of BENCH_r06.json: the optimisation step the two solves sit in


class TorchCG:
    """the same iteration, torch ops only"""

    def __init__(self, row_begin, col, lam, rtol, max_iter):
        n = len(row_begin) - 1
        dev = torch.device("cuda")
        self.A = torch.sparse_csr_tensor(torch.from_numpy(row_begin.astype(np.int64)), torch.from_numpy(col.astype(np.int64)),
                                         torch.ones(len(col), dtype=torch.float32), size=(n, n)).to(dev)
        self.lam = float(lam)
        self.d = (1.0 + self.lam * torch.from_numpy(np.diff(row_begin).astype(np.float32))).to(dev)[:, None]
        self.rtol, self.max_iter = rtol, max_iter
        self.zero = torch.zeros(3, device=dev)

    def M(self, x):
        return self.d * x - self.lam * (self.A @ x)

    def solve(self, b):
        x = torch.zeros_like(b)
        r = b.clone()
        z = r / self.d
        bb = (b * b).sum(0)
        p = torch.zeros_like(b)
        rz_old = torch.ones(3, device=b.device)
        frozen = torch.zeros(3, dtype=torch.bool, device=b.device)
        it = 0
        while it < self.max_iter:
            for _ in range(min(CHUNK, self.max_iter - it)):
                rz = (r * z).sum(0)
                frozen = frozen | ~(rz > 0)
                beta = torch.where(frozen, self.zero, rz / rz_old) if it else self.zero
                p = z + beta * p
                q = self.M(p)
                pq = (p * q).sum(0)
                frozen = frozen | ~(pq > 0)
                alpha = torch.where(frozen, self.zero, rz / pq)
                x = x + alpha * p
                r = r - alpha * q
                z = r / self.d
                rz_old = rz
                it += 1
            r = b - self.M(x)
            z = r / self.d
            norms = torch.cat([(r * r).sum(0), bb]).cpu().numpy().astype(np.float64)        # the one copy, the one synchronisation
            if np.all(np.sqrt(norms[:3]) <= self.rtol * np.sqrt(norms[3:])):
                return x, it, True
        return x, it, False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--lambda", dest="lam", type=float, default=19.0)
    ap.add_argument("--rtol", type=float, default=1e-4)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("precond_timing.py measures on the GPU: none visible")
    v, f = scenes.icosphere(opt.level, radius=150.0, noise=0.01, seed=0)
    n = int(np.asarray(v).shape[0])
    pre = psdr.LaplacianPreconditioner(np.asarray(f).reshape(-1, 3), n, lambda_=opt.lam, rtol=opt.rtol)
    ref = TorchCG(pre.row_begin, pre.col, opt.lam, opt.rtol, pre.max_iter)
    b = torch.from_numpy(np.random.default_rng(1).standard_normal((n, 3)).astype(np.float32)).cuda()

    def hip():
        x = pre._solve(b)
        return x, pre.last_solve["iterations"], pre.last_solve["converged"]

    def torch_ops():
        return ref.solve(b)

    t, last = {"hip": [], "torch": []}, {}
    for k in range(opt.warmup + opt.reps):
        for key, fn in (("hip", hip), ("torch", torch_ops)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            if k >= opt.warmup:
                t[key].append(1e3 * (time.perf_counter() - t0))
            last[key] = out
    # kernel launches of one torch-ops solve, outside the timed window
    torch_launches = None           # None: not measured (a torch build without the profiler's device tracing)
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            torch_ops()
            torch.cuda.synchronize()
        torch_launches = int(sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA
                                 and "memcpy" not in e.key.lower() and "memset" not in e.key.lower())) or None
    except Exception as exc:        # noqa: BLE001
        print("launch count of the torch form not measured: %s" % exc)
    xh, xt = last["hip"][0].double(), last["torch"][0].double()
    diff = float((xh - xt).norm() / xt.norm())
    res = {"n_vertices": n, "nnz": int(len(pre.col)), "lambda": opt.lam, "rtol": opt.rtol, "reps": opt.reps, "chunk": CHUNK, "rel_l2_between_the_two": diff,
           "step_ms_reverse_vertices": STEP_MS}
    for key in ("hip", "torch"):
        a = np.asarray(t[key])
        res[key] = {"median_ms": float(np.median(a)), "min_ms": float(a.min()), "max_ms": float(a.max()), "iterations": int(last[key][1]), "converged": bool(last[key][2])}
    res["hip"]["launches"] = int(pre.last_solve["launches"])
    res["hip"]["rel_residual"] = list(pre.last_solve["rel_residual"])
    res["torch"]["launches"] = torch_launches
    res["ratio_torch_over_hip"] = res["torch"]["median_ms"] / res["hip"]["median_ms"]
    res["two_solves_share_of_step"] = 2.0 * res["hip"]["median_ms"] / STEP_MS
    for key, name in (("hip", "psdr_hip_precond_solve"), ("torch", "torch ops only")):
        r = res[key]
        print("%-24s %8.3f ms [%8.3f, %8.3f]  %3d iterations  %5s launches  converged %s" % (name, r["median_ms"], r["min_ms"], r["max_ms"], r["iterations"], r["launches"], r["converged"]))
    print("torch / hip %.2f; two solves = %.2f %% of a %.1f ms reverse_vertices step; rel L2 between the two solutions %.1e" %
          (res["ratio_torch_over_hip"], 100.0 * res["two_solves_share_of_step"], STEP_MS, diff), flush=True)
    print(json.dumps(res))
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
