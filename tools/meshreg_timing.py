"""The mesh regularisers, value plus gradient (psdr_hip_meshreg_eval through psdr.MeshRegularizer), against the same three terms written with torch ops only - what a
user could do before it existed.  A yardstick, not a comparison against this code.

  python tools/meshreg_timing.py [--reps 30] [--warmup 5] [--out FILE.json]

Workloads: the config-5 blob (scenes.icosphere(6): 40 962 vertices), its one-level Loop subdivision (163 842) and bunny_low.obj; weights (1, 1, 1), target_length 0.05
(the edge term's general path: a square root and a division per edge).  Candidates, alternating inside one process after the warm-up:
  fused       reg.value_and_grad(v)                                           three launches
  autograd    reg(v).backward() with v a leaf                                 the same three launches behind torch's autograd engine
  torch       index_select / cross / norms / index_add_ on the same index tables, .backward() with v a leaf: its backward scatters with float atomics
Two clocks per candidate: `call` is a host clock around one call that ends in a device synchronise (median of --reps calls, min - max), what a step that reads the
loss every iteration pays; `queued` is device events around --reps calls queued back to back, divided by --reps: what the stream is busy for when nothing waits.
The table also gives whether ten gradients of the same input agree bit for bit, the relative l2 distance between the two forms' gradients, and the byte floor at the
6.29 TB/s device-copy rate DESIGN.md uses: V in (12 n bytes), the contribution buffers out and back in once (16 bytes per vertex twice, per edge once, per hinge four
times), grad out (12 n); the index tables are not counted."""
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

COPY_BYTES_PER_S = 6.29e12
WEIGHTS, L0 = (1.0, 1.0, 1.0), 0.05


class TorchForm:
    """the same definition, torch ops only"""

    def __init__(self, reg):
        dev = torch.device("cuda")
        i64 = lambda a: torch.from_numpy(np.asarray(a).astype(np.int64)).to(dev)
        t, n = reg.topology, reg.num_vertices
        self.n = n
        deg = np.diff(reg.row_begin)
        self.row, self.col = i64(np.repeat(np.arange(n), deg)), i64(reg.col)
        self.inv_deg = torch.from_numpy((1.0 / np.maximum(deg, 1)).astype(np.float32)).to(dev)[:, None]
        self.used = torch.from_numpy((deg > 0).astype(np.float32)).to(dev)[:, None]
        self.n_lap = max(int((deg > 0).sum()), 1)
        self.ea, self.eb = i64(t.edges[:, 0]), i64(t.edges[:, 1])
        self.h = [i64(t.hinges[:, k]) for k in range(4)]

    def loss(self, v):
        mean = torch.zeros_like(v).index_add_(0, self.row, v.index_select(0, self.col)) * self.inv_deg
        lap = (((v - mean) * self.used) ** 2).sum() / self.n_lap
        a, b, c, d = (v.index_select(0, k) for k in self.h)
        n1, n2 = torch.linalg.cross(b - a, c - a), torch.linalg.cross(d - a, b - a)
        u1, u2 = n1 / n1.norm(dim=1, keepdim=True).clamp_min(2.0 ** -50), n2 / n2.norm(dim=1, keepdim=True).clamp_min(2.0 ** -50)
        nor = 0.5 * ((u1 - u2) ** 2).sum() / max(len(self.h[0]), 1)
        l = (v.index_select(0, self.ea) - v.index_select(0, self.eb)).norm(dim=1)
        edge = ((l - L0) ** 2).sum() / max(len(self.ea), 1)
        return WEIGHTS[0] * lap + WEIGHTS[1] * nor + WEIGHTS[2] * edge


def floor(reg):
    n, e, h = reg.num_vertices, len(reg.topology.edges), len(reg.topology.hinges)
    contrib = 16 * (2 * n + e + 4 * h)
    total = 12 * n + 2 * contrib + 12 * n
    return {"bytes": total, "contribution_bytes": contrib, "ms": 1e3 * total / COPY_BYTES_PER_S}


def measure(name, faces, v_np, reps, warmup):
    n = int(v_np.shape[0])
    reg = psdr.MeshRegularizer(faces, n, weights=WEIGHTS, target_length=L0)
    form = TorchForm(reg)
    v = torch.from_numpy(np.ascontiguousarray(v_np, np.float32)).cuda()
    leaf = v.clone().requires_grad_()

    def fused():
        return reg.value_and_grad(v)

    def autograd():
        leaf.grad = None
        loss = reg(leaf)
        loss.backward()
        return loss.detach(), leaf.grad

    def torch_ops():
        leaf.grad = None
        loss = form.loss(leaf)
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
    topo = reg.topology
    res = {"mesh": name, "vertices": n, "edges": len(topo.edges), "hinges": len(topo.hinges), "boundary_edges": topo.num_boundary_edges,
           "nonmanifold_edges": topo.num_nonmanifold_edges, "reps": reps, "warmup": warmup, "floor": floor(reg), "bit_stable_over_10_runs": stable,
           "loss": {key: float(last[key][0]) for key, _ in cands},
           "rel_l2_gradient_vs_torch": float((last["fused"][1].double() - last["torch"][1].double()).norm() / last["torch"][1].double().norm()),
           "autograd_equals_fused": bool(torch.equal(last["fused"][1], last["autograd"][1]) and torch.equal(last["fused"][0], last["autograd"][0]))}
    print("%s: %d vertices, %d edges, %d hinges" % (name, n, len(topo.edges), len(topo.hinges)))
    for key, _ in cands:
        a = np.asarray(t[key])
        res[key] = {"call_median_ms": float(np.median(a)), "call_min_ms": float(a.min()), "call_max_ms": float(a.max()), "queued_ms": queued[key]}
        print("  %-9s call %8.4f ms [%8.4f, %8.4f]   queued %8.4f ms   bit-stable over 10 runs: %s" % (key, np.median(a), a.min(), a.max(), queued[key], stable[key]))
    f = res["floor"]
    print("  floor: %.4f ms (%d bytes, %d of them contributions); loss fused %.9g torch %.9g; gradient rel l2 against torch %.2e; autograd == fused: %s" %
          (f["ms"], f["bytes"], f["contribution_bytes"], res["loss"]["fused"], res["loss"]["torch"], res["rel_l2_gradient_vs_torch"], res["autograd_equals_fused"]), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("meshreg_timing.py measures on the GPU: none visible")
    v, f = scenes.icosphere(6, radius=150.0, noise=0.01, seed=0)
    v, f = np.asarray(v, np.float32).reshape(-1, 3) / 150.0, np.asarray(f).reshape(-1, 3)          # unit size: target_length = 0.05 is then of the edges' order
    res = [measure("config-5 blob", f, v, opt.reps, opt.warmup)]
    sub = psdr.Subdivision(f, v.shape[0], levels=1)
    res.append(measure("config-5 blob, one Loop level", sub.faces, sub.refine(torch.from_numpy(v)).cpu().numpy(), opt.reps, opt.warmup))
    bf, _bn, bv, _ft, _vt = subdiv_ref.load_obj(subdiv_ref.BUNNY)
    bv = ((bv - bv.min(0)) / (bv.max(0) - bv.min(0)).max()).astype(np.float32)
    res.append(measure("bunny_low.obj", np.asarray(bf).reshape(-1, 3), bv, opt.reps, opt.warmup))
    print(json.dumps(res))
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
