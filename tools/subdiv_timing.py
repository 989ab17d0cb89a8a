"""Subdivision's two products (psdr_hip_subdiv_apply / _apply_adj through psdr.Subdivision) against the same operator written with torch ops only - what a
user could do before it existed.  A yardstick, not a comparison against this code.

  python tools/subdiv_timing.py [--reps 30] [--warmup 5] [--out FILE.json]

Workloads, both with C = 3 and scheme "loop": bunny_low.obj at levels = 3 (2 503 -> 159 142 vertices) and the connectivity of the config-5 blob
(scenes.icosphere(6): 40 962 vertices) at levels = 1.  Candidates, alternating inside one process after the warm-up, each call timed with a host clock
around the call and a device synchronise:
  refine      sub.refine(x)                       one launch per level
  restrict    sub.restrict(y)                     one launch per level, over the stored transpose
  sparse.mm   torch.sparse.mm on the same CSR, level after level                                   (the forward a user would write)
  index_add   zeros.index_add_(0, col, w[:, None] * g.index_select(0, row)), level after level     (what autograd makes of a gather: float atomics)
The table gives the median and the min-max spread in ms, whether ten index_add gradients of the same input agree bit for bit (ours do by construction;
both are checked), the rows' lengths (one lane walks a row alone), and the floor: the bytes a direction must move - row_begin, col, weight, one read of x,
one write of y, per level - at the 6.29 TB/s device-copy rate DESIGN.md uses."""
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

COPY_BYTES_PER_S = 6.29e12
STEP_MS = 238.9          # config5.api.step_ms.reverse_vertices of BENCH_r06.json: the optimisation step of the 40 962-vertex blob
C = 3


class TorchForm:
    """the same chain, torch ops only"""

    def __init__(self, sub):
        dev = torch.device("cuda")
        self.levels = []
        for l in range(sub.levels):
            rb, col, w = sub.csr(l)
            n_out, n_in = len(rb) - 1, len(sub.csr(l, transpose=True)[0]) - 1
            A = torch.sparse_csr_tensor(torch.from_numpy(rb.astype(np.int64)), torch.from_numpy(col.astype(np.int64)), torch.from_numpy(w.copy()), size=(n_out, n_in)).to(dev)
            row = torch.from_numpy(np.repeat(np.arange(n_out, dtype=np.int64), np.diff(rb))).to(dev)
            self.levels.append((A, row, torch.from_numpy(col.astype(np.int64)).to(dev), torch.from_numpy(w.copy()).to(dev)[:, None], n_in))

    def forward(self, x):
        for A, _row, _col, _w, _n in self.levels:
            x = torch.sparse.mm(A, x)
        return x

    def backward(self, g):
        for _A, row, col, w, n_in in reversed(self.levels):
            g = torch.zeros((n_in, g.shape[1]), device=g.device, dtype=g.dtype).index_add_(0, col, w * g.index_select(0, row))
        return g


def floor_ms(sub):
    """per direction: the indices and weights of every level, one read of its input and one write of its output"""
    fwd = adj = 0
    for l in range(sub.levels):
        rb, col, _w = sub.csr(l)
        trb = sub.csr(l, transpose=True)[0]
        n_out, n_in, nnz = len(rb) - 1, len(trb) - 1, len(col)
        vec = 4 * C * (n_in + n_out)
        fwd += 4 * (n_out + 1) + 8 * nnz + vec
        adj += 4 * (n_in + 1) + 8 * nnz + vec
    return 1e3 * fwd / COPY_BYTES_PER_S, 1e3 * adj / COPY_BYTES_PER_S, fwd, adj


def row_lengths(sub):
    out = []
    for l in range(sub.levels):
        k, kt = np.diff(sub.csr(l)[0]), np.diff(sub.csr(l, transpose=True)[0])
        out.append({"level": l, "rows": int(len(k)), "nnz": int(k.sum()), "forward_median": float(np.median(k)), "forward_max": int(k.max()),
                    "transpose_median": float(np.median(kt)), "transpose_max": int(kt.max())})
    return out


def measure(name, faces, n, levels, reps, warmup):
    sub = psdr.Subdivision(faces, n, levels=levels)
    ref = TorchForm(sub)
    rng = np.random.default_rng(1)
    x = torch.from_numpy(rng.standard_normal((n, C)).astype(np.float32)).cuda()
    y = torch.from_numpy(rng.standard_normal((sub.num_vertices_out, C)).astype(np.float32)).cuda()
    cands = [("refine", lambda: sub._run(x, False, False)), ("sparse.mm", lambda: ref.forward(x)),
             ("restrict", lambda: sub._run(y, False, True)), ("index_add", lambda: ref.backward(y))]
    t, last = {k: [] for k, _ in cands}, {}
    for k in range(warmup + reps):
        for key, fn in cands:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            if k >= warmup:
                t[key].append(1e3 * (time.perf_counter() - t0))
            last[key] = out
    stable = {"index_add": all(torch.equal(ref.backward(y), last["index_add"]) for _ in range(10)),
              "restrict": all(torch.equal(sub._run(y, False, True), last["restrict"]) for _ in range(10))}
    f_ms, a_ms, f_bytes, a_bytes = floor_ms(sub)
    res = {"mesh": name, "levels": levels, "C": C, "n_in": n, "n_out": sub.num_vertices_out, "faces_out": int(sub.faces.shape[0]), "reps": reps, "warmup": warmup,
           "rows": row_lengths(sub), "floor_ms": {"refine": f_ms, "restrict": a_ms}, "floor_bytes": {"refine": f_bytes, "restrict": a_bytes},
           "bit_stable_over_10_runs": stable,
           "rel_l2_forward": float((last["refine"].double() - last["sparse.mm"].double()).norm() / last["sparse.mm"].double().norm()),
           "rel_l2_backward": float((last["restrict"].double() - last["index_add"].double()).norm() / last["index_add"].double().norm())}
    for key, _ in cands:
        a = np.asarray(t[key])
        res[key] = {"median_ms": float(np.median(a)), "min_ms": float(a.min()), "max_ms": float(a.max())}
    print("%s, levels = %d: %d -> %d vertices, %d faces" % (name, levels, n, sub.num_vertices_out, res["faces_out"]))
    for r in res["rows"]:
        print("  level %(level)d: %(rows)d rows, %(nnz)d entries; forward row median %(forward_median).0f max %(forward_max)d; transpose row median %(transpose_median).0f max %(transpose_max)d" % r)
    for key, _ in cands:
        r = res[key]
        print("  %-10s %8.4f ms [%8.4f, %8.4f]" % (key, r["median_ms"], r["min_ms"], r["max_ms"]))
    print("  floor: refine %.4f ms (%d bytes), restrict %.4f ms (%d bytes); index_add bit-stable over 10 runs: %s; restrict: %s" %
          (f_ms, f_bytes, a_ms, a_bytes, stable["index_add"], stable["restrict"]), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("subdiv_timing.py measures on the GPU: none visible")
    bunny = psdr.Mesh()
    bunny.load(os.path.join(ROOT, "examples", "data", "mesh", "bunny_low.obj"))
    res = {"bunny": measure("bunny_low.obj", np.asarray(bunny.face_indices).reshape(-1, 3), int(bunny.num_vertices), 3, opt.reps, opt.warmup)}
    v, f = scenes.icosphere(6, radius=150.0, noise=0.01, seed=0)
    res["blob"] = measure("config-5 blob", np.asarray(f).reshape(-1, 3), int(np.asarray(v).shape[0]), 1, opt.reps, opt.warmup)
    pair = res["blob"]["refine"]["median_ms"] + res["blob"]["restrict"]["median_ms"]
    res["blob"]["step_ms_reverse_vertices"] = STEP_MS
    res["blob"]["refine_plus_restrict_share_of_step"] = pair / STEP_MS
    print("config-5 blob: refine + restrict = %.4f ms = %.3f %% of a %.1f ms reverse_vertices step" % (pair, 100.0 * pair / STEP_MS, STEP_MS))
    print(json.dumps(res))
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
